"""The named relations the sigma-proof tests use throughout, in tests/sigma_twin.py's form (S, P, [(lhs, [(secret, base), ...]), ...]),
and the rows built from them.  TEST INFRASTRUCTURE ONLY."""
BB, B, SLOT = 0, 1, 16
G = lambda i: 2 + i        # noqa: E731
P_ = lambda p: SLOT + p    # noqa: E731

RELATIONS = {
    # Schnorr on an instance base: P0 = x P1.  No shared base.
    "R1": (1, 2, [(P_(0), [(0, P_(1))])]),
    # an opening: P0 = v B + r B_blinding, secrets ordered (v, r)
    "R2": (2, 1, [(P_(0), [(0, B), (1, BB)])]),
    # DLEQ: P0 = x B, P1 = x P2
    "R3": (1, 3, [(P_(0), [(0, B)]), (P_(1), [(0, P_(2))])]),
    # the same amount under two value bases: P0 = v B + r1 B_blinding, P1 = v P2 + r2 B_blinding; secrets (v, r1, r2)
    "R4": (3, 3, [(P_(0), [(0, B), (1, BB)]), (P_(1), [(0, P_(2)), (2, BB)])]),
    # the caps: S = E = 8, 32 terms, G_0 .. G_7, both Pedersen bases (twice in an equation: the coefficients add up), all 8 slots; slot 0
    # is the lhs of equation 0 and a base of equation 7
    "R5": (8, 8, [(P_(k), [(k, G(k)), ((k + 1) % 8, k % 2), ((k + 2) % 8, G((k + 3) % 8)),
                            ((k + 5) % 8, 1 - k % 2) if k < 7 else ((k + 5) % 8, P_(0))]) for k in range(8)]),
}
# R3 with the two equations' bases exchanged: the same shape, another digest
R3_SWAPPED = (1, 3, [(P_(0), [(0, P_(2))]), (P_(1), [(0, B)])])
POSITIONS = (0, 100, 150, 165)


def free_slots(rel):
    lhs = {l - SLOT for l, _ in rel[2]}
    return [p for p in range(rel[1]) if p not in lhs]


def rows(tw, bases, name, n, tag=b"", positions=POSITIONS):
    """n true statements of relation `name` with the twin's proofs: dicts of state, secrets, points, seed, proof, out"""
    rel = RELATIONS[name]
    out = []
    for i in range(n):
        key = name.encode() + tag + b"%d" % i
        secrets = [tw.det_scalar(key + b"x%d" % j, i) for j in range(rel[0])]
        free = {p: tw.msm([tw.det_scalar(key + b"h%d" % p, i)], [bases[1]]) for p in free_slots(rel)}
        pts = tw.instance(rel, bases, secrets, free)
        state = tw.state_at(positions[i % len(positions)], key)
        seed = tw.det_seed(key, i)
        proof, st, so = tw.create(state, rel, bases, pts, secrets, seed)
        assert st == tw.OK
        out.append(dict(state=state, secrets=secrets, points=pts, seed=seed, proof=proof, out=so))
    return out
