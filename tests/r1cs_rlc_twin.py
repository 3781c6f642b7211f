"""Test helper for the batch-combined R1CS check: each proof's mega-check terms as the twin verifier builds them (tests/r1cs_twin.py's
`msm`, wrapped for the duration of one verification), and the expected combination R = sum_i rho_i MegaCheck_i as ONE oracle MSM over
the concatenated weighted terms.  TEST INFRASTRUCTURE ONLY."""
import r1cs_twin as R


def verify_terms(gadget, gens, cap, st0, proof, Vs, rng32):
    """R.verify_with, plus the (scalars, points) of the proof's mega-check when it reached one (else None)"""
    seen = []
    inner = R.msm

    def capture(scalars, points):
        seen.append((list(scalars), list(points)))
        return inner(scalars, points)

    R.msm = capture
    try:
        code, mc, ts = R.verify_with(gadget, gens, cap, st0, proof, Vs, rng32)
    finally:
        R.msm = inner
    return code, mc, ts, (seen[-1] if seen else None)


def rho(weights64, i):
    return int.from_bytes(weights64[64 * i:64 * i + 64], "little") % R.L


def combination(terms, weights64):
    """compress(sum_i rho_i MegaCheck_i) over the proofs with terms (None: left out); None when a point does not decode"""
    scalars, points = [], []
    for i, t in enumerate(terms):
        if t is None:
            continue
        r = rho(weights64, i)
        scalars += [r * s % R.L for s in t[0]]
        points += t[1]
    return R.msm(scalars, points)
