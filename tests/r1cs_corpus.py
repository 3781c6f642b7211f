"""Generated R1CS gadgets (TEST INFRASTRUCTURE ONLY, like limb_corpus.py): a seeded generator of gadgets written against the common
constraint-system API, so that ONE gadget function runs unchanged on the twin Prover / Verifier (r1cs_twin.py, r1cs_prover_twin.py)
and on the product's recorders (bulletproofs_amd.r1cs.Prover / Verifier).

Satisfiable by construction, with no value tracking: every constraint that multiply() does not add itself ties a fresh allocate()
variable to an expression (its assignment is cs.eval(expr) on the twin prover, the expression itself on the recording prover, None on
verifiers), or cancels in value: k v c^e - (k - 1) v c^e - v c^e is zero as a value, not zero within a variable's list, so every entry
is weighed.  allocate_multiplier takes random free inputs.  The recorder's rules are respected: a challenge is applied one factor at
a time, a term holds one challenge, the right half of an open allocate() pair reads only variables allocated before its multiplier.

A case may pin its number of constraints and the length of its ONE list exactly: empty constraints lead (each still advances the power
of z for all that follow) and the cancelling constants open the last phase, so that the LAST constraints are ties, whose weights do
not cancel -- a cancelling constraint sits in one column at one power of z and sums to zero under any consistent error.

A case is (name, seed, shape parameters); NAMED is the fixed list whose joint coverage tests/test_r1cs_generated.py asserts from the
recorded descriptors (features()), so that the corpus cannot decay silently; sweep_case(seed) draws the shape parameters too."""
import hashlib
import random

import bp_twin as T
import r1cs_prover_twin as P
import r1cs_twin as R

L = R.L
POWERS = (1, 2, 3, 127, 128, 255)
KIND_L, KIND_R, KIND_O, KIND_V, KIND_ONE = 0, 1, 2, 3, 4


class Case:
    def __init__(self, name, seed, m=2, n1=0, n2=0, nch=0, maxpow=1, two_phase=None, labels=None, consts=True, ones=None, Q=None, extra=2,
                 script1=(), script2=(), open_end=False, cap=128):
        self.name, self.seed, self.m, self.n1, self.n2, self.nch, self.maxpow = name, seed, m, n1, n2, nch, maxpow
        self.two_phase = bool(n2 or nch or script2) if two_phase is None else two_phase
        self.labels = [b"gen challenge %d" % j for j in range(nch)] if labels is None else list(labels)
        assert len(self.labels) == nch and (self.two_phase or not (n2 or nch or script2))
        self.consts, self.ones, self.Q, self.extra = consts, ones, Q, extra      # ones / Q: exact length of the ONE list / number of constraints
        self.script1, self.script2, self.open_end, self.cap = tuple(script1), tuple(script2), open_end, cap

    def with_seed(self, seed):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.seed = seed
        return c

    def __repr__(self):
        return "Case(%s, seed %d)" % (self.name, self.seed)


def _mulpow(t, c, e):
    for _ in range(e):            # one factor at a time: the recorder takes a challenge, not a product of challenges
        t = t * c
    return t


class _Dry(R.Verifier):
    """a twin verifier that only counts: no transcript"""

    def __init__(self):
        self.constraints, self.deferred, self.num_vars, self.V, self.pending_multiplier = [], [], 0, [], None

    def challenge_scalar(self, label):
        return 1


def _plan(case, gadget):
    """how much padding reaches the case's exact number of constraints and of ONE terms: one dry run without padding counts what the
    structure itself gives (the padding draws from a stream of its own, so the structure does not depend on it)"""
    if case.Q is None and case.ones is None:
        return 0, 0
    key = (case.name, case.seed)
    if key not in _plans:
        cs = _Dry()
        st = gadget(cs, [R.Var(KIND_V, j) for j in range(case.m)], None, 0, (0, 0))
        cs.pending_multiplier = None
        for cb in cs.deferred:
            cb(cs)
        ones = 0 if case.ones is None else case.ones - st["one"]
        assert ones >= 0, (case, st)
        pad_q = sum(2 if d == 1 else 1 for d in _pad_steps(ones))
        lead = 0 if case.Q is None else case.Q - st["q"] - pad_q
        assert lead >= 0, (case, st, pad_q)
        _plans[key] = (lead, ones)
    return _plans[key]


def _pad_steps(deficit):
    """the sizes of the constraints pad_ones adds"""
    out = []
    while deficit:
        d = 1 if deficit == 1 else 2 if deficit in (2, 4) else 3
        out.append(d)
        deficit -= d
    return out


_plans = {}


def make_gadget(case):
    """gadget(cs, vs, mode, wseed): mode 'twin' (twin prover), 'rec' (recording prover), None (verifiers); wseed picks the free inputs.
    The structure depends on case.seed alone."""
    def gadget(cs, vs, mode, wseed=0, plan=None):
        plan = _plan(case, gadget) if plan is None else plan     # (empty constraints to lead with, ONE terms to pad with)
        rec = not isinstance(cs, (R.Prover, R.Verifier))
        if rec:
            from bulletproofs_amd import r1cs
            aslc, empty = r1cs._as_lc, lambda: r1cs.LinearCombination([])
        else:
            aslc, empty = R.lc, lambda: R.LC([])
        rnd = random.Random(case.seed)
        prnd = random.Random("padding %d" % case.seed)            # (its own stream: the padding does not move the structure)
        wrnd = random.Random("free %d/%d" % (case.seed, wseed))
        pool = list(vs)
        st = {"open": None, "one": 0, "q": 0}   # open: what the right half of the still-open allocate() pair may read

        def note(x):
            st["one"] += sum(1 for t in aslc(x).terms if t[0][0] == KIND_ONE)

        def constrain(x):
            note(x)
            st["q"] += 1
            cs.constrain(x)

        def multiply(a, b):
            note(a)
            note(b)
            st["q"] += 2
            out = cs.multiply(a, b)
            pool.extend(out)
            return out

        def coef():
            return rnd.choice([1, 2, L - 1, L - 2, rnd.randrange(L), rnd.randrange(1 << 64), 0])

        def power():
            return rnd.choice([p for p in POWERS if p <= case.maxpow] + [case.maxpow])

        def with_challenge(t, chs, prob):
            if chs and rnd.random() < prob:
                return _mulpow(t, rnd.choice(chs), power())
            return t

        def val(e):
            return None if mode is None else (cs.eval(e) if mode == "twin" else e)

        def free():
            a, b = wrnd.randrange(L), wrnd.randrange(1 << 32)
            return (a, b) if mode else None

        def const(chs, prob=0.5):
            return with_challenge(aslc(1 + rnd.randrange(L - 1)), chs, prob)

        def expr(chs, nterms, src=None):
            src = pool if src is None else src
            if not src:
                return const(chs)       # nothing to read yet (m = 0): a constant
            out = None
            for _ in range(nterms):
                t = with_challenge(rnd.choice(src) * coef(), chs, 0.7)
                out = t if out is None else out + t
            for _ in range(rnd.choice([0, 1, 1, 2]) if case.consts else 0):
                out = out + const(chs)
            return out

        def close_open(chs):
            if st["open"] is not None:
                lb = expr(chs, 1, st["open"])
                y = cs.allocate(val(lb))
                constrain(y - lb)
                pool.append(y)
                st["open"] = None

        def tie_pair(ea, eb):
            x = cs.allocate(val(ea))
            y = cs.allocate(val(eb))
            constrain(x - ea)
            constrain(eb - y)
            pool.extend([x, y])

        def cancel(v, chs):
            k, c, e = 2 + rnd.randrange(L - 3), (rnd.choice(chs) if chs else None), power()
            f = (lambda t: _mulpow(t, c, e)) if chs else (lambda t: t)
            constrain(f(v * k) - f(v * (k - 1)) - f(v * 1))

        def run_script(name, chs):
            close_open(chs)
            if name == "powers":       # every power of POWERS on each of L, R, O, V, ONE, coefficients other than +-1
                l, r, o = cs.allocate_multiplier(free())
                pool.extend([l, r, o])
                es = []
                for v in (l, r, o, vs[0], None):
                    for i, p in enumerate(POWERS):
                        c = chs[(-1, 0, len(chs) // 2)[i % 3]]
                        k = 2 + rnd.randrange(L - 3)
                        es.append(_mulpow(aslc(k) if v is None else v * k, c, p))
                rnd.shuffle(es)
                for i in range(0, len(es), 2):
                    tie_pair(es[i], es[i + 1])
            elif name == "wide":       # one constraint of 64+ terms
                e = expr(chs, 1)
                for _ in range(69):
                    e = e + expr(chs, 1)
                tie_pair(e, expr(chs, 2))
            elif name == "edge":       # an empty constraint, a zero coefficient, one variable twice in one constraint
                constrain(empty())
                v, w = rnd.choice(pool), rnd.choice(pool)
                tie_pair(v * 0 + w * 5, v * 3 + v * (L - 5) + w * 7 + v * 11)
                constrain(empty())
            else:
                raise ValueError(name)

        def pad_ones(chs, deficit):
            """`deficit` ONE terms in constraints that cancel in value, spread over the list: k c^e - (k - 1) c^e - c^e (or k c^e - k c^e)"""
            while deficit:
                k = 2 + prnd.randrange(L - 3)
                f = (lambda t, c=prnd.choice(chs), e=prnd.choice(POWERS[:3] + (case.maxpow,)): _mulpow(t, c, e)) if chs else (lambda t: t)
                if deficit == 1:       # a lone constant: only a tie carries it
                    tie_pair(f(aslc(k)), prnd.choice(pool) * 3 if pool else empty())
                    deficit -= 1
                elif deficit in (2, 4):
                    constrain(f(aslc(k)) - f(aslc(k)))
                    deficit -= 2
                else:
                    constrain(f(aslc(k)) - f(aslc(k - 1)) - f(aslc(1)))
                    deficit -= 3

        def body(chs, nmul, script, last):
            st["open"] = None          # the phase boundary drops an open pair (its a_R stays 0)
            if last:                   # the padding and the cancelling constraints come first, so that the last constraints are ties
                pad_ones(chs, plan[1])
            for _ in range(case.extra):
                if pool:
                    cancel(rnd.choice(pool), chs)
                elif case.consts:
                    cancel(aslc(1), chs)
            i = 0
            while i < nmul:
                kind = 3 if (case.open_end and i == nmul - 1) else rnd.randrange(4)
                if kind >= 2:
                    close_open(chs)    # the next allocate() would close the open pair: tie its right half first
                if kind == 0:
                    pool.extend(cs.allocate_multiplier(free()))
                elif kind == 1:
                    multiply(expr(chs, rnd.randrange(1, 5)), expr(chs, rnd.randrange(1, 5)))
                elif kind == 2:        # a closed allocate() pair
                    tie_pair(expr(chs, rnd.randrange(1, 5)), expr(chs, rnd.randrange(1, 5)))
                else:                  # a pair split by a multiply, closed by a later operation or left open at the end of the phase
                    la = expr(chs, 2)
                    x = cs.allocate(val(la))
                    constrain(x - la)
                    st["open"] = list(pool)     # before x joins: the recorder refuses a right half that reads its own or a later multiplier
                    pool.append(x)
                    if i + 1 < nmul:
                        multiply(expr(chs, 2), x * 3 + 1 if case.consts else x * 3)
                        i += 1
                i += 1
            for name in script:
                run_script(name, chs)

        for _ in range(plan[0]):       # empty constraints first: each still advances the power of z for everything after it
            constrain(empty())
        body([], case.n1, case.script1, not case.two_phase)
        if case.two_phase:
            def cb(cs_):
                assert cs_ is cs
                chs = [cs.challenge_scalar(lbl) for lbl in case.labels]
                body(chs, case.n2, case.script2, True)
            cs.specify_randomized_constraints(cb)
        return st
    return gadget


# ---- the named cases --------------------------------------------------------------------------------------------------------
def _labels256():
    out = [b"gen challenge %d" % j for j in range(256)]
    out[0], out[7], out[255] = b"", b"x", bytes(range(256)) * 4          # lengths 0, 1 and 1 024 (BPGPU_R1CS_MAX_LABEL)
    return out


LARGE = Case("large", 150, m=2, n1=500, n2=525, nch=2, maxpow=3, ones=2100, Q=4200, cap=2048)

NAMED = [
    Case("m_only", 101, m=2, extra=0, consts=False),                               # m > 0 == n, Q = 0, no ONE term
    Case("q1", 102, m=1, extra=1, consts=False),                                   # Q = 1
    Case("one1", 103, m=1, extra=0, consts=False, ones=1),                         # one ONE term; n = 1
    Case("n1", 104, m=0, n1=1),                                                    # m == 0 < n
    Case("n2", 105, m=1, n1=0, n2=2, nch=1, maxpow=2),                             # n1 == 0 < n2
    Case("n3", 106, m=2, n1=3, n2=0, nch=2, maxpow=3, extra=4),                    # two-phase, n2 == 0, challenges
    Case("n4", 107, m=2, n1=4, two_phase=True),                                    # two-phase with neither multipliers nor challenges
    Case("n5", 108, m=3, n1=2, n2=3, nch=8, maxpow=255),
    Case("n64", 109, m=2, n1=40, n2=24, nch=2, maxpow=128),
    Case("n65", 110, m=4, n1=1, n2=64, nch=3, maxpow=127),
    Case("q63_one31", 111, m=2, n1=3, n2=4, nch=2, maxpow=3, consts=False, ones=31, Q=63),
    Case("q64_one32", 112, m=2, n1=3, n2=4, nch=2, maxpow=255, consts=False, ones=32, Q=64),
    Case("q65_one33", 113, m=2, n1=3, n2=4, nch=2, maxpow=128, consts=False, ones=33, Q=65),
    Case("q127_one64", 114, m=3, n1=6, n2=2, nch=1, maxpow=127, consts=False, ones=64, Q=127),
    Case("q128_one65", 115, m=3, n1=5, consts=False, ones=65, Q=128),              # one-phase
    Case("q129_one0", 116, m=5, n1=2, n2=5, nch=2, maxpow=2, consts=False, ones=0, Q=129),
    Case("powers", 117, m=2, n1=2, n2=1, nch=3, maxpow=255, script2=("powers",)),
    Case("ch256", 118, m=2, n1=1, n2=2, nch=256, maxpow=255, labels=_labels256(), script2=("powers",)),
    Case("edge", 119, m=2, n1=2, n2=2, nch=2, maxpow=3, script1=("edge", "wide"), script2=("edge", "wide")),
    Case("open_ends", 120, m=2, n1=3, n2=3, nch=1, maxpow=2, open_end=True),       # a pair left open at the end of each phase
]
SMALL = list(NAMED)
NAMED = NAMED + [LARGE]


def sweep_case(seed):
    """shape parameters drawn from the seed (the structure from the same seed)"""
    rnd = random.Random("shape %d" % seed)
    n2 = rnd.choice([0, 0, 1, 2, 3, 5, 9])
    nch = rnd.choice([0, 0, 0, 1, 2, 4]) if n2 == 0 else rnd.choice([0, 1, 1, 2, 3, 8])
    return Case("sweep%d" % seed, seed, m=rnd.randrange(0, 6), n1=rnd.choice([0, 1, 2, 3, 4, 7, 12]), n2=n2, nch=nch,
                maxpow=rnd.choice([1, 2, 3, 7, 127, 128, 255]), extra=rnd.randrange(0, 4), open_end=rnd.random() < 0.25)


# ---- running a case ---------------------------------------------------------------------------------------------------------
def st0_of(case):
    return R.transcript_state(T.Transcript(b"generated gadget %d" % case.seed))


def inputs(case, idx=0):
    """the committed values and blindings of proof idx"""
    rnd = random.Random("values %d/%d" % (case.seed, idx))
    return [rnd.randrange(L) for _ in range(case.m)], [rnd.randrange(L) for _ in range(case.m)]


def prover_gadget(case, idx=0):
    g = make_gadget(case)
    return lambda cs, vs: g(cs, vs, "twin" if isinstance(cs, R.Prover) else "rec", idx)


def verifier_gadget(case):
    g = make_gadget(case)
    return lambda cs, vs: g(cs, vs, None)


def rng32_of(case, idx=0, tag=b"prove"):
    return hashlib.shake_256(b"generated rng %s %d/%d" % (tag, case.seed, idx)).digest(32)


def twin_prove(case, gens, idx=0, st0=None):
    """(proof, [V], twin prover) of proof idx of the case, with the reference's TranscriptRng over rng32_of(case, idx)"""
    vals, bl = inputs(case, idx)
    return P.prove(gens, case.cap, st0_of(case) if st0 is None else st0, vals, bl, prover_gadget(case, idx), rng32_of(case, idx))


def record_verifier(case, Vs=None, st0=None):
    from bulletproofs_amd import r1cs
    cs = r1cs.Verifier(st0_of(case) if st0 is None else st0)
    vs = [cs.commit(bytes(32) if Vs is None else Vs[j]) for j in range(case.m)]
    verifier_gadget(case)(cs, vs)
    return cs


def record_prover(case, idx=0, st0=None):
    from bulletproofs_amd import r1cs
    cs = r1cs.Prover(st0_of(case) if st0 is None else st0)
    vals, bl = inputs(case, idx)
    xs = [cs.commit(v, b) for v, b in zip(vals, bl)]
    prover_gadget(case, idx)(cs, xs)
    return cs


def features(d):
    """what a recorded descriptor reaches: the coverage the named cases are asserted to have"""
    m, n1, n2, two_phase, labels, cons = d
    terms = [t for c in cons for t in c]
    return {
        "m": m, "n1": n1, "n2": n2, "n": n1 + n2, "two_phase": bool(two_phase), "nch": len(labels), "label_lens": {len(x) for x in labels},
        "Q": len(cons), "ones": sum(1 for t in terms if t[0][0] == KIND_ONE),
        "powers": {(t[0][0], t[2]) for t in terms if t[1] is not None},
        "challenges": {t[1] for t in terms if t[1] is not None},
        "powers_coeff": {(t[0][0], t[2]) for t in terms if t[1] is not None and t[3] not in (1, L - 1)},
        "empty": any(len(c) == 0 for c in cons), "zero_coeff": any(t[3] == 0 for t in terms),
        "repeated": any(len({t[0] for t in c}) < len(c) for c in cons), "widest": max([len(c) for c in cons] + [0]),
    }


# ---- tampered proofs ----------------------------------------------------------------------------------------------------------
def tamper_cases(good, Vs):
    """(proof bytes, commitments) per exit path of verifier.rs / proof.rs; the last one is the valid proof.  The undecodable-V and
    swapped-commitment variants need one and two commitments: they are left out where there are fewer."""
    one = good[0] == 0
    nel = 11 if one else 14
    o_T = 3 if one else 6
    k = (len(good) - 1 - 32 * nel - 64) // 64
    ipp = 1 + 32 * nel
    coms = b"".join(Vs)
    cases = []
    for e in range(nel + 2 * k + 2):                  # a flipped byte in every element
        b = bytearray(good)
        b[1 + 32 * e + 7] ^= 0x10
        cases.append((bytes(b), coms))
    L_ = R.L.to_bytes(32, "little")
    for off in (1 + 32 * (o_T + 5), ipp + 64 * k, ipp + 64 * k + 32):   # t_x, a, b not canonical
        cases.append((good[:off] + L_ + good[off + 32:], coms))
    cases.append((bytes([2]) + good[1:], coms))       # bad version byte
    cases.append((good[:-1], coms))                   # bad length
    cases.append((good + bytes(64), coms))            # IPP longer than lg(padded_n)
    cases.append((good[:-128] + good[-64:], coms) if k else (good + bytes(64), coms))   # shorter
    cases.append((good[:1] + bytes(32) + good[33:], coms))                               # identity A_I1
    cases.append((good[:1 + 32 * (o_T + 1)] + bytes(32) + good[1 + 32 * (o_T + 2):], coms))   # identity T_3
    if k:
        cases.append((good[:ipp] + bytes(32) + good[ipp + 32:], coms))                   # identity L_0
    if len(Vs) >= 1:
        cases.append((good, b"\xff" * 32 + coms[32:]))    # undecodable V
    if len(Vs) >= 2:
        cases.append((good, coms[32:] + coms[:32]))       # swapped commitments
    cases.append((good, coms))
    return cases
