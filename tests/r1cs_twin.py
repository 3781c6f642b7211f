"""Test-side restatement of the reference's R1CS prover and verifier (src/r1cs/prover.rs, src/r1cs/verifier.rs) and of the
gadgets of its tests (tests/r1cs.rs): the parity anchor of the GPU R1CS verifier.  There is no golden R1CS vector anywhere
(the reference's `yoloproofs` feature is off, Cargo.toml:43), so proofs are synthesised here.

Built on oracle/py/bp_twin.py (Merlin / STROBE-128, scalars) with the STROBE KEY operation and merlin's TranscriptRng added
below; every multiscalar multiplication goes through the C oracle's oracle_msm (liboracle.so) on compressed encodings, so
that padded_n = 2048 proofs take seconds.  TEST INFRASTRUCTURE ONLY: the product never imports this file.
"""
import bp_twin as T
import pyoracle as O

L = T.L
KIND_L, KIND_R, KIND_O, KIND_V, KIND_ONE = 0, 1, 2, 3, 4
IDENTITY = bytes(32)


def sc_bytes(s):
    return (s % L).to_bytes(32, "little")


def msm(scalars, points):
    """sum scalars[i] * points[i] over compressed encodings (oracle_msm); None when a point does not decode"""
    st, out = O.msm(b"".join(sc_bytes(s) for s in scalars), b"".join(points))
    return None if st else out


# ---- merlin 2.x extras: a transcript from / to its 208-byte state, STROBE KEY, TranscriptRng ----------------------------
def transcript_from_state(state):
    t = T.Transcript.__new__(T.Transcript)
    s = T.Strobe128.__new__(T.Strobe128)
    s.st = bytearray(state[:200])
    s.pos, s.pos_begin, s.cur_flags = state[200], state[201], state[202]
    t.strobe = s
    return t


def transcript_state(t):
    s = t.strobe
    return bytes(s.st) + bytes([s.pos, s.pos_begin, s.cur_flags]) + bytes(5)


def strobe_key(s, data):
    """strobe.rs key(): begin_op(A | C), then overwrite the state bytes"""
    s._begin_op(s.FLAG_A | s.FLAG_C, False)
    for b in data:
        s.st[s.pos] = b
        s.pos += 1
        if s.pos == s.R:
            s._run_f()


def transcript_rng_scalar(t, rng32):
    """Scalar::random(&mut t.build_rng().finalize(rng)) with rng yielding rng32 (merlin 2 transcript.rs: build_rng clones the
    strobe; finalize: meta_ad(b"rng"), key(32 random bytes); fill_bytes: meta_ad(u32le(len)), prf(len)).  t is not advanced."""
    s = t.strobe.clone()
    s.meta_ad(b"rng", False)
    strobe_key(s, rng32)
    s.meta_ad((64).to_bytes(4, "little"), False)
    return int.from_bytes(s.prf(64), "little") % L


# ---- variables / linear combinations (src/r1cs/linear_combination.rs): terms [((kind, index), coeff)] -----------------
def lc(x):
    if isinstance(x, LC):
        return x
    if isinstance(x, Var):
        return LC([((x.kind, x.index), 1)])
    if isinstance(x, int):
        return LC([((KIND_ONE, 0), x % L)])
    raise TypeError(x)


class _Ops:
    def __add__(self, o):
        return LC(lc(self).terms + lc(o).terms)

    def __radd__(self, o):
        return lc(o) + self

    def __sub__(self, o):
        return self + lc(o) * -1

    def __rsub__(self, o):
        return lc(o) + lc(self) * -1

    def __neg__(self):
        return lc(self) * -1

    def __mul__(self, k):
        assert isinstance(k, int)
        return LC([(v, c * k % L) for v, c in lc(self).terms])

    __rmul__ = __mul__


class Var(_Ops):
    def __init__(self, kind, index):
        self.kind, self.index = kind, index


class LC(_Ops):
    def __init__(self, terms):
        self.terms = list(terms)


# ---- Prover (src/r1cs/prover.rs) ------------------------------------------------------------------------------------------
class Prover:
    def __init__(self, gens, transcript, seed=b"prover"):
        self.gens = gens                      # (G bytes, H bytes, B, B_blinding) as pyoracle.Gens.export()
        self.G, self.H = gens[0], gens[1]
        self.B, self.Bb = gens[2], gens[3]
        self.t = transcript
        self.t.append_message(b"dom-sep", b"r1cs v1")     # Prover::new (prover.rs:277-282)
        self.constraints, self.deferred = [], []
        self.a_L, self.a_R, self.a_O = [], [], []
        self.v, self.v_blinding = [], []
        self.pending_multiplier = None
        self.rng = T.ShakeRng(seed)

    def eval(self, x):
        out = 0
        for (k, i), c in lc(x).terms:
            val = {KIND_L: self.a_L, KIND_R: self.a_R, KIND_O: self.a_O, KIND_V: self.v}.get(k)
            out += c * (1 if k == KIND_ONE else val[i])
        return out % L

    def commit(self, v, v_blinding):                      # prover.rs:296-306
        i = len(self.v)
        self.v.append(v % L)
        self.v_blinding.append(v_blinding % L)
        V = msm([v, v_blinding], [self.B, self.Bb])
        self.t.append_point(b"V", V)
        return V, Var(KIND_V, i)

    def multiply(self, left, right):                      # prover.rs:101-124
        l, r = self.eval(left), self.eval(right)
        i = len(self.a_L)
        self.a_L.append(l)
        self.a_R.append(r)
        self.a_O.append(l * r % L)
        lv, rv, ov = Var(KIND_L, i), Var(KIND_R, i), Var(KIND_O, i)
        self.constrain(lc(left) - lv)
        self.constrain(lc(right) - rv)
        return lv, rv, ov

    def allocate(self, assignment):                       # prover.rs:126-146
        if self.pending_multiplier is None:
            i = len(self.a_L)
            self.pending_multiplier = i
            self.a_L.append(assignment % L)
            self.a_R.append(0)
            self.a_O.append(0)
            return Var(KIND_L, i)
        i, self.pending_multiplier = self.pending_multiplier, None
        self.a_R[i] = assignment % L
        self.a_O[i] = self.a_L[i] * self.a_R[i] % L
        return Var(KIND_R, i)

    def allocate_multiplier(self, assignments):          # prover.rs:148-165
        l, r = assignments
        i = len(self.a_L)
        self.a_L.append(l % L)
        self.a_R.append(r % L)
        self.a_O.append(l * r % L)
        return Var(KIND_L, i), Var(KIND_R, i), Var(KIND_O, i)

    def constrain(self, x):
        self.constraints.append(lc(x))

    def specify_randomized_constraints(self, cb):
        self.deferred.append(cb)

    def challenge_scalar(self, label):
        return self.t.challenge_scalar(label)

    def flattened(self, z):                               # prover.rs:341-381
        n, m = len(self.a_L), len(self.v)
        w = {KIND_L: [0] * n, KIND_R: [0] * n, KIND_O: [0] * n, KIND_V: [0] * m}
        ez = z
        for c in self.constraints:
            for (k, i), coeff in c.terms:
                if k == KIND_V:
                    w[k][i] = (w[k][i] - ez * coeff) % L
                elif k != KIND_ONE:
                    w[k][i] = (w[k][i] + ez * coeff) % L
            ez = ez * z % L
        return w[KIND_L], w[KIND_R], w[KIND_O], w[KIND_V]

    def prove(self, gens_capacity):                       # prover.rs:410-655
        self.t.append_u64(b"m", len(self.v))
        n1 = len(self.a_L)
        if gens_capacity < n1:
            raise T.InvalidGeneratorsLength()
        r_ = self.rng.scalar
        i_b1, o_b1, s_b1 = r_(), r_(), r_()
        sL1 = [r_() for _ in range(n1)]
        sR1 = [r_() for _ in range(n1)]
        G, H = self.G, self.H
        g = lambda i: G[32 * i:32 * i + 32]
        h = lambda i: H[32 * i:32 * i + 32]
        A_I1 = msm([i_b1] + self.a_L + self.a_R, [self.Bb] + [g(i) for i in range(n1)] + [h(i) for i in range(n1)])
        A_O1 = msm([o_b1] + self.a_O, [self.Bb] + [g(i) for i in range(n1)])
        S1 = msm([s_b1] + sL1 + sR1, [self.Bb] + [g(i) for i in range(n1)] + [h(i) for i in range(n1)])
        self.t.append_point(b"A_I1", A_I1)
        self.t.append_point(b"A_O1", A_O1)
        self.t.append_point(b"S1", S1)
        # create_randomized_constraints (prover.rs:384-407)
        self.pending_multiplier = None
        if not self.deferred:
            self.t.append_message(b"dom-sep", b"r1cs-1phase")
        else:
            self.t.append_message(b"dom-sep", b"r1cs-2phase")
            for cb in self.deferred:
                cb(self)
            self.deferred = []
        n = len(self.a_L)
        n2 = n - n1
        pn = next_pow2(n)
        pad = pn - n
        if gens_capacity < pn:
            raise T.InvalidGeneratorsLength()
        if n2 > 0:
            i_b2, o_b2, s_b2 = r_(), r_(), r_()
        else:
            i_b2 = o_b2 = s_b2 = 0
        sL2 = [r_() for _ in range(n2)]
        sR2 = [r_() for _ in range(n2)]
        if n2 > 0:
            gi = [g(i) for i in range(n1, n)]
            hi = [h(i) for i in range(n1, n)]
            A_I2 = msm([i_b2] + self.a_L[n1:] + self.a_R[n1:], [self.Bb] + gi + hi)
            A_O2 = msm([o_b2] + self.a_O[n1:], [self.Bb] + gi)
            S2 = msm([s_b2] + sL2 + sR2, [self.Bb] + gi + hi)
        else:
            A_I2 = A_O2 = S2 = IDENTITY
        self.t.append_point(b"A_I2", A_I2)
        self.t.append_point(b"A_O2", A_O2)
        self.t.append_point(b"S2", S2)
        y = self.t.challenge_scalar(b"y")
        z = self.t.challenge_scalar(b"z")
        wL, wR, wO, wV = self.flattened(z)
        y_inv = T.sc_inv(y)
        exp_y_inv = [pow(y_inv, i, L) for i in range(pn)]
        sL, sR = sL1 + sL2, sR1 + sR2
        l1, l2, l3, r0, r1, r3 = [0] * n, [0] * n, [0] * n, [0] * n, [0] * n, [0] * n
        exp_y = 1
        for i in range(n):
            l1[i] = (self.a_L[i] + exp_y_inv[i] * wR[i]) % L
            l2[i] = self.a_O[i]
            l3[i] = sL[i]
            r0[i] = (wO[i] - exp_y) % L
            r1[i] = (exp_y * self.a_R[i] + wL[i]) % L
            r3[i] = exp_y * sR[i] % L
            exp_y = exp_y * y % L
        ip = T.inner_product                                  # VecPoly3::special_inner_product (util.rs:127-145)
        t1 = ip(l1, r0)
        t2 = (ip(l1, r1) + ip(l2, r0)) % L
        t3 = (ip(l2, r1) + ip(l3, r0)) % L
        t4 = (ip(l1, r3) + ip(l3, r1)) % L
        t5 = ip(l2, r3)
        t6 = ip(l3, r3)
        tb = [r_() for _ in range(5)]
        Ts = [msm([tv, bl], [self.B, self.Bb]) for tv, bl in zip((t1, t3, t4, t5, t6), tb)]
        for lbl, P in zip((b"T_1", b"T_3", b"T_4", b"T_5", b"T_6"), Ts):
            self.t.append_point(lbl, P)
        u = self.t.challenge_scalar(b"u")
        x = self.t.challenge_scalar(b"x")
        t2b = sum(c * vb for c, vb in zip(wV, self.v_blinding)) % L
        poly6 = lambda c: x * (c[0] + x * (c[1] + x * (c[2] + x * (c[3] + x * (c[4] + x * c[5]))))) % L
        t_x = poly6((t1, t2, t3, t4, t5, t6))
        t_x_blinding = poly6((tb[0], t2b, tb[1], tb[2], tb[3], tb[4]))
        l_vec = [(x * (l1[i] + x * (l2[i] + x * l3[i]))) % L for i in range(n)] + [0] * pad
        r_vec = [(r0[i] + x * (r1[i] + x * x * r3[i])) % L for i in range(n)] + [0] * pad
        for i in range(n, pn):
            r_vec[i] = -exp_y % L
            exp_y = exp_y * y % L
        i_bl = (i_b1 + u * i_b2) % L
        o_bl = (o_b1 + u * o_b2) % L
        s_bl = (s_b1 + u * s_b2) % L
        e_blinding = x * (i_bl + x * (o_bl + x * s_bl)) % L
        self.t.append_scalar(b"t_x", t_x)
        self.t.append_scalar(b"t_x_blinding", t_x_blinding)
        self.t.append_scalar(b"e_blinding", e_blinding)
        w = self.t.challenge_scalar(b"w")
        Q = msm([w], [self.B])
        G_factors = [1] * n1 + [u] * (n2 + pad)
        H_factors = [yi * gf % L for yi, gf in zip(exp_y_inv, G_factors)]
        ipp = ipp_create(self.t, Q, G_factors, H_factors, [g(i) for i in range(pn)], [h(i) for i in range(pn)], l_vec, r_vec)
        return Proof([A_I1, A_O1, S1, A_I2, A_O2, S2] + Ts, t_x, t_x_blinding, e_blinding, ipp)


def ipp_create(t, Q, Gf, Hf, G, H, a, b):
    """InnerProductProof::create (inner_product_proof.rs:38-193); the folded generators are kept as coefficients on the
    ORIGINAL ones, so every L_j / R_j is one multiscalar multiplication over G, H, Q (the same group elements)."""
    n = len(G)
    t.innerproduct_domain_sep(n)
    gc, hc = list(Gf), list(Hf)
    a, b = list(a), list(b)
    Ls, Rs = [], []
    size = n
    while size != 1:
        h = size // 2
        aL, aR, bL, bR = a[:h], a[h:], b[:h], b[h:]
        cL, cR = T.inner_product(aL, bR), T.inner_product(aR, bL)
        ls, lp, rs, rp = [], [], [], []
        for o in range(n):
            c = o % size
            if c >= h:
                ls.append(aL[c - h] * gc[o])
                lp.append(G[o])
                rs.append(bL[c - h] * hc[o])
                rp.append(H[o])
            else:
                ls.append(bR[c] * hc[o])
                lp.append(H[o])
                rs.append(aR[c] * gc[o])
                rp.append(G[o])
        Lp = msm(ls + [cL], lp + [Q])
        Rp = msm(rs + [cR], rp + [Q])
        Ls.append(Lp)
        Rs.append(Rp)
        t.append_point(b"L", Lp)
        t.append_point(b"R", Rp)
        u = t.challenge_scalar(b"u")
        ui = T.sc_inv(u)
        a = [(aL[i] * u + ui * aR[i]) % L for i in range(h)]
        b = [(bL[i] * ui + u * bR[i]) % L for i in range(h)]
        for o in range(n):
            left = o % size < h
            gc[o] = gc[o] * (ui if left else u) % L
            hc[o] = hc[o] * (u if left else ui) % L
        size = h
    return b"".join(x + y for x, y in zip(Ls, Rs)) + sc_bytes(a[0]) + sc_bytes(b[0])


def next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


class Proof:
    def __init__(self, pts, t_x, t_x_blinding, e_blinding, ipp):
        self.pts, self.t_x, self.t_x_blinding, self.e_blinding, self.ipp = pts, t_x, t_x_blinding, e_blinding, ipp

    def to_bytes(self, force_two_phase=False):            # proof.rs:75-110
        one = all(p == IDENTITY for p in self.pts[3:6]) and not force_two_phase
        pts = self.pts[:3] + self.pts[6:] if one else self.pts
        return bytes([0 if one else 1]) + b"".join(pts) + sc_bytes(self.t_x) + sc_bytes(self.t_x_blinding) + sc_bytes(self.e_blinding) + self.ipp


# ---- Verifier (src/r1cs/verifier.rs) ----------------------------------------------------------------------------------------
OK, VERIFICATION_ERROR, FORMAT_ERROR, INVALID_GENERATORS_LENGTH = 0, 1, 2, 4


class _Stop(Exception):
    def __init__(self, code):
        self.code = code


class Verifier:
    def __init__(self, transcript):
        self.t = transcript
        self.t.append_message(b"dom-sep", b"r1cs v1")     # verifier.rs:189-194
        self.constraints, self.deferred = [], []
        self.num_vars = 0
        self.V = []
        self.pending_multiplier = None

    def commit(self, V):                                  # verifier.rs:235-243
        self.V.append(V)
        self.t.append_point(b"V", V)
        return Var(KIND_V, len(self.V) - 1)

    def multiply(self, left, right):                      # verifier.rs:67-87
        i = self.num_vars
        self.num_vars += 1
        lv, rv, ov = Var(KIND_L, i), Var(KIND_R, i), Var(KIND_O, i)
        self.constrain(lc(left) - lv)
        self.constrain(lc(right) - rv)
        return lv, rv, ov

    def allocate(self, assignment=None):                  # verifier.rs:89-102
        if self.pending_multiplier is None:
            i = self.num_vars
            self.num_vars += 1
            self.pending_multiplier = i
            return Var(KIND_L, i)
        i, self.pending_multiplier = self.pending_multiplier, None
        return Var(KIND_R, i)

    def allocate_multiplier(self, assignments=None):     # verifier.rs:104-118
        i = self.num_vars
        self.num_vars += 1
        return Var(KIND_L, i), Var(KIND_R, i), Var(KIND_O, i)

    def constrain(self, x):
        self.constraints.append(lc(x))

    def specify_randomized_constraints(self, cb):
        self.deferred.append(cb)

    def challenge_scalar(self, label):                    # verifier.rs:175-179
        return self.t.challenge_scalar(label)

    def flattened(self, z):                               # verifier.rs:260-298
        n, m = self.num_vars, len(self.V)
        w = {KIND_L: [0] * n, KIND_R: [0] * n, KIND_O: [0] * n, KIND_V: [0] * m, KIND_ONE: [0]}
        ez = z
        for c in self.constraints:
            for (k, i), coeff in c.terms:
                if k in (KIND_V, KIND_ONE):
                    w[k][i] = (w[k][i] - ez * coeff) % L
                else:
                    w[k][i] = (w[k][i] + ez * coeff) % L
            ez = ez * z % L
        return w[KIND_L], w[KIND_R], w[KIND_O], w[KIND_V], w[KIND_ONE][0]

    def verify(self, proof_bytes, gens, gens_capacity, rng32):
        """-> (verdict, mega-check encoding or None); self.t is left as the reference leaves it"""
        try:
            return OK if self._verify(parse(proof_bytes), gens, gens_capacity, rng32) else VERIFICATION_ERROR, self.msm
        except _Stop as e:
            return e.code, None

    def _validate(self, label, P):
        if P == IDENTITY:
            raise _Stop(VERIFICATION_ERROR)
        self.t.append_point(label, P)

    def _verify(self, pr, gens, gens_capacity, rng32):    # verifier.rs:329-500
        self.msm = None
        t = self.t
        t.append_u64(b"m", len(self.V))
        n1 = self.num_vars
        self._validate(b"A_I1", pr["A_I1"])
        self._validate(b"A_O1", pr["A_O1"])
        self._validate(b"S1", pr["S1"])
        self.pending_multiplier = None
        if not self.deferred:
            t.append_message(b"dom-sep", b"r1cs-1phase")
        else:
            t.append_message(b"dom-sep", b"r1cs-2phase")
            for cb in self.deferred:
                cb(self)
            self.deferred = []
        n = self.num_vars
        n2 = n - n1
        pn = next_pow2(n)
        pad = pn - n
        if gens_capacity < pn:
            raise _Stop(INVALID_GENERATORS_LENGTH)
        t.append_point(b"A_I2", pr["A_I2"])
        t.append_point(b"A_O2", pr["A_O2"])
        t.append_point(b"S2", pr["S2"])
        y = t.challenge_scalar(b"y")
        z = t.challenge_scalar(b"z")
        for lbl in (b"T_1", b"T_3", b"T_4", b"T_5", b"T_6"):
            self._validate(lbl, pr[lbl.decode()])
        u = t.challenge_scalar(b"u")
        x = t.challenge_scalar(b"x")
        t.append_scalar(b"t_x", pr["t_x"])
        t.append_scalar(b"t_x_blinding", pr["t_x_blinding"])
        t.append_scalar(b"e_blinding", pr["e_blinding"])
        w = t.challenge_scalar(b"w")
        wL, wR, wO, wV, wc = self.flattened(z)
        # verification_scalars(padded_n) (inner_product_proof.rs:198-253)
        Lv, Rv = pr["L"], pr["R"]
        k = len(Lv)
        if pn != (1 << k):
            raise _Stop(VERIFICATION_ERROR)
        t.innerproduct_domain_sep(pn)
        us = []
        for Li, Ri in zip(Lv, Rv):
            self._validate(b"L", Li)
            self._validate(b"R", Ri)
            us.append(t.challenge_scalar(b"u"))
        u_inv = [T.sc_inv(v) for v in us]
        s = []
        for i in range(pn):
            acc = 1
            for j in range(k):
                acc = acc * (us[j] if (i >> (k - 1 - j)) & 1 else u_inv[j]) % L
            s.append(acc)
        a, b = pr["a"], pr["b"]
        y_inv = T.sc_inv(y)
        yiv = [pow(y_inv, i, L) for i in range(pn)]
        yneg_wR = [wR[i] * yiv[i] % L for i in range(n)] + [0] * pad
        delta = T.inner_product(yneg_wR[:n], wL)
        u_for = [1] * n1 + [u] * (n2 + pad)
        wLp, wOp = wL + [0] * pad, wO + [0] * pad
        g_sc = [u_for[i] * (x * yneg_wR[i] - a * s[i]) % L for i in range(pn)]
        h_sc = [u_for[i] * (yiv[i] * (x * wLp[i] + wOp[i] - b * s[pn - 1 - i]) - 1) % L for i in range(pn)]
        r = transcript_rng_scalar(t, rng32)
        xx = x * x % L
        rxx = r * xx % L
        xxx = x * xx % L
        T_sc = [r * x, rxx * x, rxx * xx, rxx * xxx, rxx * xx * xx]
        scal = [x, xx, xxx, u * x, u * xx, u * xxx] + [v * rxx for v in wV] + T_sc + \
               [w * (pr["t_x"] - a * b) + r * (xx * (wc + delta) - pr["t_x"]), -pr["e_blinding"] - r * pr["t_x_blinding"]] + \
               g_sc + h_sc + [v * v for v in us] + [v * v for v in u_inv]
        G, H, B, Bb = gens
        pts = [pr["A_I1"], pr["A_O1"], pr["S1"], pr["A_I2"], pr["A_O2"], pr["S2"]] + self.V + \
              [pr[l] for l in ("T_1", "T_3", "T_4", "T_5", "T_6")] + [B, Bb] + \
              [G[32 * i:32 * i + 32] for i in range(pn)] + [H[32 * i:32 * i + 32] for i in range(pn)] + Lv + Rv
        self.msm = msm(scal, pts)
        if self.msm is None:
            raise _Stop(VERIFICATION_ERROR)
        return self.msm == IDENTITY


def parse(b):
    """R1CSProof::from_bytes (proof.rs:129-204) -> dict; raises _Stop(FORMAT_ERROR)"""
    if len(b) < 1 or (len(b) - 1) % 32 or b[0] not in (0, 1):
        raise _Stop(FORMAT_ERROR)
    nel = 11 if b[0] == 0 else 14
    rest = b[1:]
    if len(rest) < 32 * nel:
        raise _Stop(FORMAT_ERROR)
    el = [rest[32 * i:32 * i + 32] for i in range(nel)]
    if b[0] == 0:
        el = el[:3] + [IDENTITY] * 3 + el[3:]
    d = dict(zip(("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6"), el[:11]))
    for nm, e in zip(("t_x", "t_x_blinding", "e_blinding"), el[11:]):
        v = int.from_bytes(e, "little")
        if v >= L:
            raise _Stop(FORMAT_ERROR)
        d[nm] = v
    ipp = rest[32 * nel:]
    ne = len(ipp) // 32
    if ne < 2 or (ne - 2) % 2 or (ne - 2) // 2 >= 32:
        raise _Stop(FORMAT_ERROR)
    k = (ne - 2) // 2
    d["L"] = [ipp[64 * i:64 * i + 32] for i in range(k)]
    d["R"] = [ipp[64 * i + 32:64 * i + 64] for i in range(k)]
    for nm, e in (("a", ipp[64 * k:64 * k + 32]), ("b", ipp[64 * k + 32:64 * k + 64])):
        v = int.from_bytes(e, "little")
        if v >= L:
            raise _Stop(FORMAT_ERROR)
        d[nm] = v
    return d


def flattened_with(gadget, m, z, challenges):
    """the twin verifier's flattened(z) for `gadget` with its challenge draws replaced by the given values: (wL, wR, wO, wV, wc).
    As verifier.rs:300-321, an allocate() pair still open at the end of phase 1 is dropped before the deferred callbacks run."""
    class Fixed(Verifier):
        def __init__(self):
            self.constraints, self.deferred, self.num_vars, self.V, self.pending_multiplier = [], [], 0, [], None
            self.draws = list(challenges)

        def challenge_scalar(self, label):
            return self.draws.pop(0)

    cs = Fixed()
    cs.V = [bytes(32)] * m
    gadget(cs, [Var(KIND_V, i) for i in range(m)])
    cs.pending_multiplier = None
    for cb in cs.deferred:
        cb(cs)
    return cs.flattened(z)


# ---- the gadgets of tests/r1cs.rs, generic over the constraint system ------------------------------------------------------
def shuffle_gadget(cs, x, y):                             # tests/r1cs.rs:22-58
    k = len(x)
    if k == 1:
        cs.constrain(y[0] - x[0])
        return

    def cb(cs):
        z = cs.challenge_scalar(b"shuffle challenge")
        _, _, last_mulx_out = cs.multiply(x[k - 1] - z, x[k - 2] - z)
        prev = last_mulx_out
        for i in reversed(range(k - 2)):
            _, _, prev = cs.multiply(prev, x[i] - z)
        first_mulx_out = prev
        _, _, last_muly_out = cs.multiply(y[k - 1] - z, y[k - 2] - z)
        prev = last_muly_out
        for i in reversed(range(k - 2)):
            _, _, prev = cs.multiply(prev, y[i] - z)
        cs.constrain(first_mulx_out - prev)

    cs.specify_randomized_constraints(cb)


def example_gadget(cs, a1, a2, b1, b2, c1, c2):          # tests/r1cs.rs:233-244
    _, _, c_var = cs.multiply(a1 + a2, b1 + b2)
    cs.constrain(c1 + c2 - c_var)


def range_gadget(cs, v, v_assignment, n):                 # tests/r1cs.rs:370-395
    exp_2 = 1
    for i in range(n):
        if v_assignment is None:
            a, b, o = cs.allocate_multiplier(None)
        else:
            bit = (v_assignment >> i) & 1
            a, b, o = cs.allocate_multiplier((1 - bit, bit))
        cs.constrain(o)
        cs.constrain(a + (b - 1))
        v = v - b * exp_2
        exp_2 = exp_2 + exp_2
    cs.constrain(v)


# ---- proof synthesis helpers --------------------------------------------------------------------------------------------
def prove_shuffle(gens, cap, label, inp, out, seed):
    """ShuffleProof::prove (tests/r1cs.rs:61-100): (proof, commitments of inputs + outputs, transcript state before Verifier::new)"""
    t = T.Transcript(label)
    k = len(inp)
    t.append_message(b"dom-sep", b"ShuffleProof")
    t.append_u64(b"k", k)
    st0 = transcript_state(t)
    P = Prover(gens, t, seed)
    rng = T.ShakeRng(seed + b"/blinding")
    xs, ys, Vs = [], [], []
    for v in inp:
        V, var = P.commit(v, rng.scalar())
        Vs.append(V)
        xs.append(var)
    for v in out:
        V, var = P.commit(v, rng.scalar())
        Vs.append(V)
        ys.append(var)
    shuffle_gadget(P, xs, ys)
    return P.prove(cap), Vs, st0


def _parses(proof_bytes):
    """R1CSProof::from_bytes runs before Verifier::new: a proof it rejects leaves the caller's transcript untouched"""
    try:
        parse(proof_bytes)
        return True
    except _Stop:
        return False


def verify_shuffle(gens, cap, st0, proof_bytes, Vs, rng32):
    if not _parses(proof_bytes):
        return FORMAT_ERROR, None, st0
    t = transcript_from_state(st0)
    V = Verifier(t)
    vars_ = [V.commit(c) for c in Vs]
    k = len(Vs) // 2
    shuffle_gadget(V, vars_[:k], vars_[k:])
    code, mc = V.verify(proof_bytes, gens, cap, rng32)
    return code, mc, transcript_state(t)


def prove_example(gens, cap, vals, c2, seed):
    """example_gadget_proof (tests/r1cs.rs:246-279): vals = (a1, a2, b1, b2, c1)"""
    t = T.Transcript(b"R1CSExampleGadget")
    st0 = transcript_state(t)
    P = Prover(gens, t, seed)
    rng = T.ShakeRng(seed + b"/blinding")
    Vs, vs = [], []
    for v in vals:
        V, var = P.commit(v, rng.scalar())
        Vs.append(V)
        vs.append(var)
    example_gadget(P, vs[0], vs[1], vs[2], vs[3], vs[4], c2)
    return P.prove(cap), Vs, st0


def prove_range(gens, cap, v, n, seed):
    """range_proof_helper's prover half (tests/r1cs.rs:421-440)"""
    t = T.Transcript(b"RangeProofTest")
    st0 = transcript_state(t)
    P = Prover(gens, t, seed)
    V, var = P.commit(v, T.ShakeRng(seed + b"/blinding").scalar())
    range_gadget(P, var, v, n)
    return P.prove(cap), [V], st0


def verify_with(gadget, gens, cap, st0, proof_bytes, Vs, rng32):
    """run `gadget(cs, vars)` on a fresh twin Verifier over transcript state st0 and verify"""
    if not _parses(proof_bytes):
        return FORMAT_ERROR, None, st0
    t = transcript_from_state(st0)
    V = Verifier(t)
    vars_ = [V.commit(c) for c in Vs]
    gadget(V, vars_)
    code, mc = V.verify(proof_bytes, gens, cap, rng32)
    return code, mc, transcript_state(t)
