// R1CS witness check on the device: which constraint of a recorded gadget does a witness leave unsatisfied?  Constraint q of
// proof p holds iff Prover::eval(lc_q) == 0 (src/r1cs/prover.rs:340-356 of the reference): the sum over the row's terms of
// coeff * ch_j^power * value, mod l, with value = a_L[i], a_R[i], a_O[i], v_j or 1.
//   r1c_chal_thread  : lane = (proof, challenge)   the stand-alone form's challenge values: canonical? -> Montgomery form at f_ch
//   r1c_unit_thread  : lane = (unit, proof), proof fastest   at most R1C_CHUNK term products: a whole row (reported at once) or
//                                        one chunk of a long row (its partial sum parked)
//   r1c_long_thread  : lane = (long row, proof)   the parked partial sums of one long row added up, then reported
// SIGN: the row form holds the coefficients as the gadget recorded them, i.e. the per-variable lists' sign flip on V and ONE
// (r1cs_build_lists) is undone, so a residual is exactly Prover::eval's value.
// The rows run over what the prover's launches leave behind: a_L, a_R, a_O in `aw`, the phase-2 challenges in `fields`
// (r1cs_prover.h); r1p_term_product is the witness rows' own term product.
// Reporting: failing lanes alone touch first / count / map, with 32-bit atomics whose results do not depend on arrival order
// (min, add, or).  A proof whose status word is set already (a non-canonical input) is not checked.
#ifndef BPGPU_R1CS_CHECK_H
#define BPGPU_R1CS_CHECK_H
#include "r1cs_prover.h"
#include <algorithm>

namespace bp {

// Term products per lane.  Gadget rows are short: multiply's two rows have a handful of terms, the shuffle's rows two or three;
// the longest row of a common gadget is the range gadget's closing row v - sum 2^i b_i with n + 1 terms, 65 for 64 bits.  At 128
// that row is still finished by its own lane and touches no partial sum, where 32 or 64 would send it through the partial buffer
// and a second launch; 256 would only lengthen the slowest lane of a launch over hand-built long rows.
#define R1C_CHUNK 128
#define R1C_SATISFIED 0xffffffffu
#define R1C_NO_SLOT 0xffffffffu
#define R1C_STATUS_UNSATISFIED 3u          // BPGPU_R1CS_UNSATISFIED
#define R1C_SLICE 1024                     // proofs per slice of a circuit with long rows (as R1_RLC_SLICE) ...
#define R1C_PART_BYTES ((size_t)64 << 20)  // ... or fewer: the partial sums of one slice stay within this

// terms [t0, t1) of constraint q; slot: where a long row's chunk parks its partial sum (R1C_NO_SLOT: the whole row, reported here)
struct r1c_unit {
    uint32_t q, t0, t1, slot;
};
// a row of more than R1C_CHUNK terms: its chunks' partial sums sit in slots [slot0, slot0 + nchunk)
struct r1c_long {
    uint32_t q, slot0, nchunk;
};

// constraint q of proof p failed
BP_HD void r1c_report(uint32_t q, uint32_t p, uint32_t mapw, uint32_t *first, uint32_t *count, uint32_t *map) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(first + p, q);
    if (count) atomicAdd(count + p, 1u);
    if (map) atomicOr(map + (uint64_t)p * mapw + (q >> 5), 1u << (q & 31u));
#else
    if (first[p] > q) first[p] = q;
    if (count) count[p] += 1u;
    if (map) map[(uint64_t)p * mapw + (q >> 5)] |= 1u << (q & 31u);
#endif
}

// lane = (proof, j): challenge j of proof p from 32 bytes (nproofs x nch x 32, draw order)
BP_HD void r1c_chal_thread(uint32_t tid, const r1p_shape &sh, const uint8_t *chal, uint32_t *fields, uint32_t *status) {
    const uint32_t p = tid / sh.c.nch, j = tid - p * sh.c.nch;
    sc c;
    sc28 cm;
    r1p_ld_bytes(c, chal + (uint64_t)tid * 32);
    if (!sc_is_canonical_sc(c)) {
        status_raise(status + p, BP_STATUS_BAD_SCALAR);
        sc_0(c);
    }
    sc_to_mont28(cm, c);
    r1_store28(fields, sh.c, sh.c.f_ch + j, p, cm);
}

// lane = (unit, proof) over proofs [p0, p0 + cnt) of the batch; partial: [slot][proof of the slice][8 words]
BP_HD void r1c_unit_thread(uint32_t tid, const r1p_shape &sh, uint32_t p0, uint32_t cnt, const r1c_unit *units, const r1p_term *terms, const uint32_t *aw,
                           const uint8_t *v, const uint32_t *fields, const uint32_t *status, uint32_t mapw, uint32_t *partial, uint32_t *first,
                           uint32_t *count, uint32_t *map) {
    const uint32_t u = tid / cnt, pl = tid - u * cnt, p = p0 + pl;
    if (status[p] != 0) return;
    const r1c_unit un = units[u];
    sc acc;
    sc_0(acc);
    for (uint32_t t = un.t0; t < un.t1; t++) {
        sc s;
        r1p_term_product(s, sh, terms[t], aw, v, fields, p);
        sc_add(acc, acc, s);
    }
    if (un.slot != R1C_NO_SLOT) {
        store_words8(partial + ((uint64_t)un.slot * cnt + pl) * 8, acc);
        return;
    }
    if (!words8_zero(acc.v)) r1c_report(un.q, p, mapw, first, count, map);
}

// lane = (long row, proof) over the same slice
BP_HD void r1c_long_thread(uint32_t tid, uint32_t p0, uint32_t cnt, const r1c_long *longs, const uint32_t *partial, const uint32_t *status, uint32_t mapw,
                           uint32_t *first, uint32_t *count, uint32_t *map) {
    const uint32_t l = tid / cnt, pl = tid - l * cnt, p = p0 + pl;
    if (status[p] != 0) return;
    const r1c_long lg = longs[l];
    sc acc, s;
    sc_0(acc);
    for (uint32_t k = 0; k < lg.nchunk; k++) {
        const uint32_t *src = partial + ((uint64_t)(lg.slot0 + k) * cnt + pl) * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) s.v[q] = src[q];
        sc_add(acc, acc, s);
    }
    if (!words8_zero(acc.v)) r1c_report(lg.q, p, mapw, first, count, map);
}

// ---- host side: the row form of a circuit, from the per-variable lists bpgpu_r1cs_circuit_create keeps (libbpgpu.so and the host
// harness of tests/r1cs_check_harness run the same functions) ----------------------------------------------------------------------
struct r1c_rows {
    std::vector<r1p_term> terms;     // CSR: the terms of constraint 0, 1, ..
    std::vector<r1c_unit> units;
    std::vector<r1c_long> longs;
    uint32_t nslots = 0;             // partial sums per proof (the chunks of the long rows)
};
inline void r1c_build_rows(size_t m, size_t n, size_t Q, const std::vector<uint32_t> &col_ptr, const std::vector<r1cs_ent> &ents, r1c_rows &out) {
    std::vector<uint32_t> row_ptr(Q + 1, 0);
    for (const r1cs_ent &e : ents) row_ptr[e.q + 1]++;
    for (size_t q = 0; q < Q; q++) row_ptr[q + 1] += row_ptr[q];
    out.terms.resize(ents.size());
    std::vector<uint32_t> fill(row_ptr.begin(), row_ptr.end() - 1);
    const size_t ncols = 3 * n + m + 1;
    for (size_t col = 0; col < ncols; col++)
        for (uint32_t t = col_ptr[col]; t < col_ptr[col + 1]; t++) {
            const r1cs_ent &s = ents[t];
            r1p_term &e = out.terms[fill[s.q]++];
            e.kind = (uint32_t)(col < 3 * n ? col % 3 : col < 3 * n + m ? 3 : 4);
            e.index = (uint32_t)(col < 3 * n ? col / 3 : col < 3 * n + m ? col - 3 * n : 0);
            e.chal = s.chal;
            sc28 cm;
            sc cf;
            memcpy(cm.v, s.coeff, 40);
            sc_from_mont28(cf, cm);
            if (e.kind >= 3) sc_neg(cf, cf);   // the lists hold -coeff for V and ONE
            sc_to_mont28(cm, cf);
            memcpy(e.coeff, cm.v, 40);
        }
    out.units.clear();
    out.longs.clear();
    out.nslots = 0;
    for (size_t q = 0; q < Q; q++) {
        const uint32_t t0 = row_ptr[q], t1 = row_ptr[q + 1], len = t1 - t0;
        if (len <= R1C_CHUNK) {
            out.units.push_back(r1c_unit{(uint32_t)q, t0, t1, R1C_NO_SLOT});
            continue;
        }
        const uint32_t nchunk = (len + R1C_CHUNK - 1) / R1C_CHUNK;
        out.longs.push_back(r1c_long{(uint32_t)q, out.nslots, nchunk});
        for (uint32_t k = 0; k < nchunk; k++) {
            const uint32_t a = t0 + k * R1C_CHUNK;
            out.units.push_back(r1c_unit{(uint32_t)q, a, a + R1C_CHUNK < t1 ? a + R1C_CHUNK : t1, out.nslots++});
        }
    }
}
// proofs per slice of a batch: the whole batch unless the lane count of a launch or the partial sums of the long rows bound it
inline size_t r1c_slice(const r1c_rows &rows, size_t nbatch) {
    size_t per = nbatch;
    if (rows.nslots) per = std::min(per, std::max<size_t>(1, std::min<size_t>(R1C_SLICE, R1C_PART_BYTES / ((size_t)rows.nslots * 32))));
    if (!rows.units.empty()) per = std::min(per, std::max<size_t>(1, ((size_t)1 << 30) / rows.units.size()));
    return std::max<size_t>(per, 1);
}

}  // namespace bp
#endif
