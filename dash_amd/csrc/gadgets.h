// Garbled gates and gadgets shared by the host garbler and the host (oracle)
// evaluator. Every gadget is written per *element* (one neuron across all CRT
// residues) so that the garbler, the CPU evaluator and the HIP kernels all
// walk exactly the same sequence of gates and table offsets.
//
// Reference behaviour reproduced here (semantics, not code):
//   projection gate           garbling/gates/projection_gate.h:62-102
//   mini projection           garbling/gates/projection_gate_mini.h:25-56
//   generalized half gate     garbling/gates/generalized_half_gate.h:51-89
//   mixed-modulus half gate   garbling/gates/mixed_mod_half_gate.h:56-104
//   approx-residue lookup     garbling/gadgets/lookup_approx_sign.h:75-101
//   approximate sign gadget   garbling/gadgets/sign_gadget.h:425-671
//   rescale gadget            garbling/gadgets/rescale_gadget.h:115-362
//   base extension gadget     garbling/gadgets/base_extension_gadget.h:70-295
// Table layouts are element-major (see docs/WIRE_FORMAT.md); the reference's
// residue-major rescale layout (rescale_gadget.h:152-175) is not reproduced
// because its own GPU kernel could not read it.
#pragma once

#include "core.h"

namespace dash {

// ---------------------------------------------------------------------------
// Offset (R_p) and zero (Z_p) labels for every modulus 2..max_modulus.
// ---------------------------------------------------------------------------
struct LabelBank {
    int max_mod = 0;
    std::vector<std::vector<comp_t>> lab;  // indexed by modulus
    const comp_t* get(int p) const {
        DASH_CHECK(p >= 2 && p <= max_mod && !lab[p].empty(), "label bank has no entry for modulus " + std::to_string(p));
        return lab[p].data();
    }
};

// ---------------------------------------------------------------------------
// Projection gate
// ---------------------------------------------------------------------------
struct ProjScratch {
    std::vector<comp_t> key, tmp;
    std::vector<u128> kc, hc, payc;
    std::vector<int> colors;
    std::vector<uint8_t> have;
};
ProjScratch& proj_scratch();

// Colors and hashes of the p keys in0 + i*Rin of one input label; shared by
// every projection of that label (the approx step projects one residue label
// into all t MRS digits: one key schedule instead of t).
// The keys of one projection row: kc[i] = compress(in0 + i*Rin), hc[i] = H(kc[i]) (reference masks), and
// per key the hardened pads of the row's tweak, one block at a time (pads of a fan-out row's slots)
struct ProjKeys {
    std::vector<comp_t> key;
    std::vector<u128> kc, hc;
    std::vector<int> colors;
    std::vector<PadRow> pads;
    bool hard = false;
    // mask of key i for mask m (m.hard: pad m.slot of (kc[i], m.gate, m.sub))
    u128 mask(int i, const Mask& m) {
        if (!m.hard) return hc[i];
        PadRow& r = pads[i];
        if (r.gate != m.gate || r.sub != m.sub || r.blk < 0) r = PadRow(kc[i], m.gate, m.sub);
        return r.get(m.slot);
    }
};
// hard: skip the reference hashes (hardened rows use the pads only)
inline void proj_keys(const comp_t* in0, const comp_t* Rin, const ModInfo& mi, ProjKeys& K, bool hard = false) {
    const int pin = mi.p, nin = mi.n;
    K.key.assign(in0, in0 + nin);
    K.kc.resize(pin);
    K.hc.resize(pin);
    K.colors.resize(pin);
    K.hard = hard;
    for (int i = 0; i < pin; ++i) {
        K.kc[i] = compress(K.key.data(), mi);
        K.colors[i] = K.key[0];
        lab_add(K.key.data(), Rin, nin, pin);
    }
    if (hard) K.pads.assign(pin, PadRow());
    else hash_batch(K.kc.data(), K.hc.data(), pin);
}

// table[color(in0 + i*Rin) * stride] = compress(out0 + f(i)*outR) + mask(compress(in0 + i*Rin))
template <class F>
inline void garble_proj_keys(ProjKeys& K, const comp_t* out0, const comp_t* outR, const ModInfo& mo, F&& f,
                             u128* table, int stride = 1, const Mask& mk = Mask()) {
    ProjScratch& s = proj_scratch();
    const int pin = static_cast<int>(K.kc.size());
    s.payc.resize(mo.p);
    s.have.assign(mo.p, 0);
    s.tmp.resize(mo.n);
    for (int i = 0; i < pin; ++i) {
        int c = static_cast<int>(pmod(f(i), mo.p));
        if (!s.have[c]) {
            lab_affine(s.tmp.data(), out0, c, outR, mo.n, mo.p);
            s.payc[c] = compress(s.tmp.data(), mo);
            s.have[c] = 1;
        }
        table[static_cast<i64>(K.colors[i]) * stride] = s.payc[c] + K.mask(i, mk);
    }
}

ProjKeys& proj_keys_scratch();

template <class F>
inline void garble_proj(const comp_t* in0, const comp_t* Rin, const ModInfo& mi, const comp_t* out0,
                        const comp_t* outR, const ModInfo& mo, F&& f, u128* table, int stride = 1,
                        const Mask& mk = Mask()) {
    ProjKeys& K = proj_keys_scratch();
    proj_keys(in0, Rin, mi, K, mk.hard);
    garble_proj_keys(K, out0, outR, mo, std::forward<F>(f), table, stride, mk);
}

// Mini projection: 16-bit payloads t16[color] = f(i) + mask16. Reference: the low 16 bits of H(K), the same
// hash the key's full-entry projection uses (projection_gate_mini.h); hardened: lane `lane` (16 bits) of the
// pad of mk.slot, a slot no full entry of the row uses.
template <class F>
inline void garble_proj_mini(const comp_t* in0, const comp_t* Rin, const ModInfo& mi, F&& f, u128* entry,
                             const Mask& mk = Mask(), int lane = 0) {
    ProjScratch& s = proj_scratch();
    const int pin = mi.p, nin = mi.n;
    DASH_CHECK(pin <= 8, "mini projection supports input moduli <= 8");
    s.key.assign(in0, in0 + nin);
    int16_t* t16 = reinterpret_cast<int16_t*>(entry);
    for (int i = 0; i < pin; ++i) {
        const u128 kc = compress(s.key.data(), mi);
        const u128 h = mk.hard ? (hard_pad(kc, mk.gate, mk.sub, mk.slot) >> (16 * lane)) : hash(kc);
        int color = s.key[0];
        t16[color] = static_cast<int16_t>(static_cast<int16_t>(f(i)) + static_cast<int16_t>(static_cast<uint16_t>(h)));
        lab_add(s.key.data(), Rin, nin, pin);
    }
}

inline int color_of(const comp_t* L, int p) { return static_cast<int>(static_cast<uint16_t>(L[0]) % static_cast<unsigned>(p)); }

// out = decompress(T[color(in) * stride] - mask(compress(in)))
inline void eval_proj(const comp_t* in, const ModInfo& mi, const u128* table, const ModInfo& mo, comp_t* out,
                      int stride = 1, const Mask& mk = Mask()) {
    const u128 kc = compress(in, mi);
    const u128 h = mk.hard ? hard_pad(kc, mk.gate, mk.sub, mk.slot) : hash(kc);
    decompress(table[static_cast<i64>(color_of(in, mi.p)) * stride] - h, out, mo);
}

inline int16_t eval_proj_mini(const comp_t* in, const ModInfo& mi, const u128* entry, const Mask& mk = Mask(),
                              int lane = 0) {
    const u128 kc = compress(in, mi);
    const u128 h = mk.hard ? (hard_pad(kc, mk.gate, mk.sub, mk.slot) >> (16 * lane)) : hash(kc);
    const int16_t* t16 = reinterpret_cast<const int16_t*>(entry);
    return static_cast<int16_t>(t16[color_of(in, mi.p)] - static_cast<int16_t>(static_cast<uint16_t>(h)));
}

// ---------------------------------------------------------------------------
// Approximate sign gadget (per element)
// ---------------------------------------------------------------------------
//
// Two constructions of the same function (SignPlan::fused):
//  * reference (fused = false): per digit d >= 1 every residue's approx label
//    (mod m_d) and the carry (mod m_d) are cast to Z_{(k+1) m_d} by identity
//    projections before the sum (sign_gadget.h:456-546): k + 1 casts per digit;
//  * fused (fused = true): the casts are folded into the projections that
//    produce their inputs. The approx projection of residue j writes digit d
//    directly as a label mod (k+1) m_d (value lut[j][v][d] < m_d), and the
//    carry projection of digit d writes (floor(s / m_d) mod m_{d-1}) directly
//    mod (k+1) m_{d-1} (mod m_0 for the last carry). The least significant
//    digit has no carry-in (the reference adds a cast of the zero label).
//    Every wire carries the same value as in the reference construction, so
//    the gadget computes the same function; it uses k (t-1) + (t-1) fewer
//    projections per element (k = 7, t = 5: 44 -> 12 hashes and table reads
//    on the evaluator side; the cast1 table disappears).
struct SignPlan {
    std::vector<int> crt, mrs, out_mod;
    int lower = 0, upper = 1;
    bool fused = false;
    std::vector<std::vector<int16_t>> lookup;  // [k][v * t + d], d = 0 is most significant
    std::vector<i64> crt_prefix;
    i64 sum_crt = 0;
    i64 n_approx = 0, n_cast = 0, n_sign = 0;  // table entries per element (n_cast: cast2; cast1 too unless fused)
    int max_n = 0;                             // largest label width touched

    SignPlan() = default;
    SignPlan(const std::vector<int>& crt_, const std::vector<int>& mrs_, const std::vector<int>& out, int lo, int up,
             bool fused = false);
    // modulus of residue j's approx output for digit d (and of the digit-d sums)
    int digit_mod(int d) const { return (fused && d >= 1) ? static_cast<int>(crt.size() + 1) * mrs[d] : mrs[d]; }
    // modulus of the carry produced by digit d >= 1 (consumed by digit d - 1)
    int carry_mod(int d) const { return fused ? ((d - 1 >= 1) ? static_cast<int>(crt.size() + 1) * mrs[d - 1] : mrs[0]) : mrs[d - 1]; }
    bool has_cast1() const { return !fused; }
};

std::vector<std::vector<int16_t>> gen_approx_lookup(const std::vector<int>& crt, const std::vector<int>& mrs);

// Garbler: in0[j] = base label of residue j (mod crt[j]); out0[o] receives the
// output base label for out_mod[o].
// hard: hardened masks (core.h Mask) with gate = the gadget's PRG stream `stream` (the evaluator passes the
// same value as `gate`); the hardened encoding needs the fused construction (no constant-keyed carry cast)
void sign_garble_elem(const SignPlan& P, const LabelBank& R, const LabelBank& Z, const Prg& prg, u64 stream,
                      const comp_t* const* in0, u128* approx, u128* cast1, u128* cast2, u128* sign,
                      comp_t* const* out0, bool hard = false);
void sign_eval_elem(const SignPlan& P, const LabelBank& Z, const comp_t* const* in, const u128* approx,
                    const u128* cast1, const u128* cast2, const u128* sign, comp_t* const* out, bool hard = false,
                    u64 gate = 0);

// ---------------------------------------------------------------------------
// Mixed-modulus half gate x (mod p) * y (mod q), q <= 8. Tables: g[p], e[q+1].
// ---------------------------------------------------------------------------
// Hardened tweaks of one mixed half gate (gate = the gadget's PRG stream): the garbler half's key x_j is row
// (TW_MMG, j); the evaluator half's key y is row (TW_MMY, 0) shared by the k residues of a ReLU (shared_y:
// residue j's entry at slot j, its mini at lane j % 8 of slot k + j / 8), or row (TW_MMY, j) of its own
// (entry at slot 0, mini at lane 0 of slot 1)
struct MMTw {
    bool hard = false;
    u64 gate = 0;
    int j = 0, k = 1;
    bool shared_y = true;
    Mask g() const { return Mask{hard, gate, tw_sub(TW_MMG, j), 0}; }
    Mask e() const { return Mask{hard, gate, tw_sub(TW_MMY, shared_y ? 0 : j), shared_y ? j : 0}; }
    Mask mini() const { return Mask{hard, gate, tw_sub(TW_MMY, shared_y ? 0 : j), shared_y ? k + j / 8 : 1}; }
    int lane() const { return shared_y ? j % 8 : 0; }
};
void mixed_mult_garble(const comp_t* x0, const ModInfo& mp, const comp_t* y0, const ModInfo& mq,
                       const LabelBank& R, const Prg& prg, u64 stream, u64& ctr, u128* g, u128* e, comp_t* out0,
                       const MMTw& tw = MMTw());
void mixed_mult_eval(const comp_t* x, const ModInfo& mp, const comp_t* y, const ModInfo& mq, const u128* g,
                     const u128* e, comp_t* out, const MMTw& tw = MMTw());

// Generalized half gate x * y, both mod p. Tables g[p], e[p].
void gen_mult_garble(const comp_t* x0, const comp_t* y0, const ModInfo& mp, const LabelBank& R, const Prg& prg,
                     u64 stream, u64& ctr, u128* g, u128* e, comp_t* out0, bool hard = false, int j = 0);
void gen_mult_eval(const comp_t* x, const comp_t* y, const ModInfo& mp, const u128* g, const u128* e, comp_t* out,
                   bool hard = false, u64 gate = 0, int j = 0);

// ---------------------------------------------------------------------------
// Base extension (ReDash MRS conversion) per element
// ---------------------------------------------------------------------------
struct BEPlan {
    std::vector<int> moduli;        // output (full) base, length E
    std::vector<int> extra;         // moduli to (re)derive
    std::vector<int> extra_idx;     // their indices in `moduli`
    std::vector<int> swapped;       // moduli order used by the MRS loop
    std::vector<int> pos_of;        // for every base index i: position in swapped
    std::vector<std::vector<i64>> inv_partial;  // [i][j] = inv(b_i) mod b_{i+j+1}
    std::vector<i64> invv;          // per extra modulus
    int nonext = 0;
    i64 n_tab = 0;                  // table entries per element
    BEPlan() = default;
    BEPlan(const std::vector<int>& moduli, const std::vector<int>& extra);
};
// L[j] are labels (mod moduli[j]) of one element, updated in place.
void be_garble_elem(const BEPlan& P, const LabelBank& R, const Prg& prg, u64 stream, u64& ctr, comp_t* const* L,
                    u128* tab, bool hard = false);
void be_eval_elem(const BEPlan& P, comp_t* const* L, const u128* tab, bool hard = false, u64 gate = 0);

// ---------------------------------------------------------------------------
// Rescale gadget (one iteration) per element.
//   legacy: factors = {2}, residue 0 recovered by a sign gadget (out {2}, 1/0)
//   redash: factors = s (subset of the CRT base), recovered by base extension
// ---------------------------------------------------------------------------
struct RescalePlan {
    std::vector<int> crt;
    std::vector<int> factors;
    std::vector<int> factor_idx;
    bool sign_be = true;
    i64 n_trans = 0;  // trans-mod entries per element
    std::vector<std::vector<int>> active;  // per factor: residues processed
    std::vector<std::vector<i64>> inv;     // per factor, per active residue: inv(s) mod p
    SignPlan sign;                         // when sign_be
    BEPlan be;                             // otherwise
    i64 n_be = 0;
    i64 sprod = 1;
    RescalePlan() = default;
    RescalePlan(const std::vector<int>& crt, const std::vector<int>& mrs, const std::vector<int>& factors, bool sign_be,
                bool fused_sign = false);
};
// Garbler: L[j] base labels (mod crt[j]) in/out; up/down are the garbler-side
// (offset-free) shift base labels.
void rescale_garble_elem(const RescalePlan& P, const LabelBank& R, const LabelBank& Z, const Prg& prg, u64 stream,
                         comp_t* const* L, const comp_t* const* up_base, const comp_t* const* down_base, u128* trans,
                         u128* s_approx, u128* s_cast1, u128* s_cast2, u128* s_sign, u128* be, bool hard = false);
void rescale_eval_elem(const RescalePlan& P, const LabelBank& Z, comp_t* const* L, const comp_t* const* up,
                       const comp_t* const* down, const u128* trans, const u128* s_approx, const u128* s_cast1,
                       const u128* s_cast2, const u128* s_sign, const u128* be, bool hard = false, u64 gate = 0);

// ---------------------------------------------------------------------------
// Single-shot mixed-radix rescale (the DASH legacy function, new construction)
//
// The legacy gadget divides by S = 2^l with l iterations of "subtract the
// mod-2 residue, halve, recover residue 0 with a sign gadget" (rescale_gadget.h
// :115-242, each iteration a full approximate sign gadget). Composed, the l
// iterations compute y = ceil(x / S) (Rescale._apply). Here the same y comes
// from one exact mixed-radix conversion:
//   x_u = (x + U) mod M with U = S - 1 + S q, U >= M/2 (U ~ M/2)
//   MRS digits a_i of x_u over the CRT base (crt[0] = 2, ascending order):
//     digit i: key K_i = L_i - sum_{l<i} P_{l,i}, a_i = (v_i + U) B_i^-1 mod p_i
//     its table row fans out P_{i,j} = a_i B_i mod p_j to every later residue j
//     and P_{i,T} = a_i B_i mod T (T = 2S) to a power-of-two label
//   r = sum_i P_{i,T} = x_u mod 2S (free additions)
//   final row (T entries): residue j >= 1: Y_j = S^-1 L_j + [(U - r mod S) S^-1 - q]
//                          residue 0:      Y_0 = [(floor(r / S) - q) mod 2]
// so y = floor(x_u / S) - q = ceil(x / S) for every x in [-M/2, M/2 - (U - M/2)):
// only the top U - M/2 < S values of the signed range wrap (they differ from
// the legacy gadget). k + 1 hashes and table reads per element on the
// evaluator instead of l sign gadgets (l = 5, k = 7: 8 instead of ~60), and
// sum_i p_i (k - i) + T k table entries instead of l (2 (k - 1) + sign).
// Table (one row per element): digit i at dig_off[i], [color][k - i] entries
// (targets: the residues of positions i+1..k-1, then T); final rows at
// fin_off, [color][k] (targets: residues 0..k-1).
//
// sign_last (the joint rescale + ReLU sign): positions convert residues
// 1..k-1 and residue 0 (mod 2) LAST, as SignMrsPlan. Its digit a_{k-1} has
// weight B_{k-1} = M/2, so a_{k-1} = [x_u >= M/2] = [x >= M/2 - U] with
// M/2 - U in (-S, 0]; with U mod 2 folded into digit 0's payload for residue
// 0, residue 0's key after the k-1 subtractions IS the label of a_{k-1}. For
// the ReLU that follows, relu(y) = y * a_{k-1} with y = ceil(x / S): y >= 1
// means x >= 1 (sign 1), y <= -1 means x <= -S (sign 0), and y = 0 gives 0
// either way, so the rescale's conversion replaces the ReLU's sign gadget.
// The last position's row has one target (T) and takes a_{k-1} as is.
struct RescaleMrsPlan {
    std::vector<int> crt;
    int l = 0;
    bool sign_last = false;
    i64 S = 1, T = 2, M = 1, U = 0, q = 0;
    std::vector<int> ord;     // position -> residue (identity, or 1..k-1, 0 with sign_last)
    std::vector<i64> B;       // B[i] = prod_{m<i} crt[ord[m]]
    std::vector<i64> Binv;    // B[i]^-1 mod crt[ord[i]]
    std::vector<i64> Sinv;    // S^-1 mod crt[j] (j >= 1)
    std::vector<i64> dig_off; // table offset of digit i's rows
    i64 fin_off = 0, n_tab = 0;
    RescaleMrsPlan() = default;
    RescaleMrsPlan(const std::vector<int>& crt, int l, bool sign_last = false);
    int k() const { return static_cast<int>(crt.size()); }
    int targets(int i) const { return k() - i; }
    // residue of target t < k-1-i of digit i (position i + 1 + t)
    int target_res(int i, int t) const { return ord[i + 1 + t]; }
    // modulus of target t of digit i (residue of position i + 1 + t, the last one T)
    int target_mod(int i, int t) const { return t == k() - 1 - i ? static_cast<int>(T) : crt[ord[i + 1 + t]]; }
    // payload value of digit i, target t, for key value v (a_i B_i reduced mod the target modulus)
    i64 digit_fn(int i, int t, i64 v) const;
    // payload value of final target j for key value v = x_u mod T
    i64 final_fn(int j, i64 v) const;
    // the smallest input x with output floor((x + U) / S) - q >= y
    i64 min_input(i64 y) const { return (y + q) * S - U; }
};
// L[j] (one element's labels mod crt[j]) are replaced by the rescaled labels;
// with sign_last, sig (nullable) receives the mod-2 label of a_{k-1}.
void rescale_mrs_garble_elem(const RescaleMrsPlan& P, const LabelBank& R, const Prg& prg, u64 stream,
                             comp_t* const* L, u128* tab, comp_t* sig = nullptr, bool hard = false);
void rescale_mrs_eval_elem(const RescaleMrsPlan& P, comp_t* const* L, const u128* tab, comp_t* sig = nullptr,
                           bool hard = false, u64 gate = 0);

// ---------------------------------------------------------------------------
// Exact sign by mixed-radix conversion (a construction of the ReLU/Sign
// gadget's sign; the reference approximates it, sign_gadget.h:425-581)
//
// With residue 0 = 2 converted LAST, x_u = x + M/2 = sum_i a_i B_i and the
// last digit's weight is B_{k-1} = M/2, so a_{k-1} = [x_u >= M/2] = [x >= 0]
// exactly. Positions 0..k-2 convert residues 1..k-1 (ascending); digit i's
// table row fans its value a_i B_i out to the later residues (the constant
// -M/2 is folded into digit 0's payload for residue 0), and residue 0's key
// after the k-1 subtractions IS the sign label (mod 2) - no table of its own.
// k-1 hashes on the critical path; sum_{i<k-1} p_{i+1} (k-1-i) table entries
// (k = 7: 147 instead of the approximate gadget's 568) and exact for every x.
// Rows: position i at dig_off[i], [color][k-1-i] (targets: positions i+1..k-1).
struct SignMrsPlan {
    std::vector<int> crt;
    std::vector<int> ord;      // position -> residue: 1, 2, ..., k-1, 0
    i64 M = 1, U = 0;
    std::vector<i64> B, Binv;  // per position: product of the earlier positions' moduli; its inverse mod p
    std::vector<i64> dig_off;
    i64 n_tab = 0;
    SignMrsPlan() = default;
    explicit SignMrsPlan(const std::vector<int>& crt);
    int k() const { return static_cast<int>(crt.size()); }
    int targets(int i) const { return k() - 1 - i; }
    int target_res(int i, int t) const { return ord[i + 1 + t]; }
    i64 digit_fn(int i, int t, i64 v) const;
};
// sign01 base label (mod 2) of one element with residue base labels x0; tables at tab
void sign_mrs_garble_elem(const SignMrsPlan& P, const LabelBank& R, const Prg& prg, u64 stream,
                          const comp_t* const* x0, u128* tab, comp_t* sig0, bool hard = false);
void sign_mrs_eval_elem(const SignMrsPlan& P, const comp_t* const* x, const u128* tab, comp_t* sig, bool hard = false,
                        u64 gate = 0);

// ---------------------------------------------------------------------------
// Clip (clamp to public bounds q_lo < q_hi; ONNX Clip, ReLU6) per element
//
// Two signs of the same input and one multiply, instead of the two complete
// ReLU gadgets of relu(x - lo) - relu(x - hi):
//   s_lo = [x >= q_lo], s_hi = [x >= q_hi]   (mod-2 labels)
// each from a sign gadget run on the SAME evaluator labels x_j: the public
// shifts -q_lo / -q_hi are folded into the garbler's base labels of the two
// gadgets (x0_j + q R_j is the base of the wire x - q with unchanged labels),
// so the evaluator runs the sign evaluation twice, with two table sets, on one
// input and does no shift work. The signs are the approximate fused gadget
// (SignPlan, out {2}, 0/1) or the exact SignMrsPlan; both are exact on
// x - q in [-M/2, M/2) up to the approximate gadget's own error.
// q_hi > q_lo, so s_hi = 1 implies s_lo = 1 and the free label sum
//   u = s_lo + s_hi (mod 2) = [q_lo <= x < q_hi].
//   out_j = q_lo + u (x_j - q_lo) + s_hi (q_hi - q_lo)   (mod p_j)
// The product is the mixed-modulus half gate of the ReLU keyed by the label of
// u, on the wire x_j - q_lo (again a base-label fold): p_j garbler rows, 2
// evaluator rows and the mini. The last term ("cap") is a 2-row projection
// Z_2 -> Z_{p_j} keyed by the label of s_hi; q_lo is folded into the output
// base label. Hardened encoding only: the folds are the hardened encoding's
// public-constant rule, and the labels of u and s_hi each key k rows, which
// needs the per-(gate, row, slot) pads (TW_MMY as the ReLU, TW_CAP slot j).
// Tables: the two sign gadgets' arrays under "lo." / "hi.", mm.g [sum p_j],
// mm.e [k][3], cap [k][2] (row = color of s_hi). Entries per element, with
// n_sign the sign gadget's entries (approx: n_approx + n_cast + n_sign; exact:
// SignMrsPlan::n_tab) and P = sum_j p_j:
//   clip      2 n_sign + P + 3 k + 2 k
//   two ReLUs 2 n_sign + 2 P + 6 k
// (k = 7, first primes: exact 294 + 58 + 35 = 387 against 452.)
// PRG streams: sign lo = slot 1, multiply and cap = slot 2 (the cap's base
// label is drawn after the k half gates' draws), sign hi = slot 3.
//
// Joint variant (a Clip(0, q_hi) directly behind a mixed-radix rescale with
// sign_last, input x, output y = ceil(x / S)): s_lo is the rescale's own sign
// label a_{k-1} = [x >= M/2 - U] (it differs from [y >= 0] only where y = 0,
// where u y = 0 either way, as for the joint ReLU), and s_hi = [y >= q_hi] =
// [x >= t_hi] is one exact SignMrsPlan sign of the wire x - t_hi on the
// rescale's INPUT labels, t_hi = the smallest x the rescale maps to q_hi
// (RescaleMrsPlan::min_input). t_hi >= 1 > M/2 - U, so s_hi = 1 still implies
// s_lo = 1. The multiply and the cap run on y_j unchanged. Tables: hi.mrs,
// mm.g, mm.e, cap; n_sign + P + 5 k entries. Domain: x - t_hi >= -M/2.
struct ClipPlan {
    std::vector<int> crt;
    i64 lo = 0, hi = 1;
    i64 sum_crt = 0;
    std::vector<i64> prefix;  // mm.g offset of residue j
    bool joint = false;
    i64 t_hi = 0;  // joint: threshold of the upper sign on the rescale's input
    ClipPlan() = default;
    ClipPlan(const std::vector<int>& crt_, i64 lo_, i64 hi_) : crt(crt_), lo(lo_), hi(hi_) {
        DASH_CHECK(lo < hi, "clip needs lo < hi");
        for (int p : crt) {
            prefix.push_back(sum_crt);
            sum_crt += p;
        }
    }
    // the joint variant behind the rescale `rs`
    ClipPlan(const std::vector<int>& crt_, i64 hi_, const RescaleMrsPlan& rs) : ClipPlan(crt_, 0, hi_) {
        DASH_CHECK(rs.sign_last, "joint clip needs a sign-producing rescale");
        joint = true;
        t_hi = rs.min_input(hi);
    }
    int k() const { return static_cast<int>(crt.size()); }
    // table entries per element given the sign gadget's entry count
    i64 entries(i64 n_sign) const { return (joint ? 1 : 2) * n_sign + sum_crt + 3 * k() + 2 * k(); }
    static i64 two_relu_entries(i64 n_sign, i64 sum_crt, int k) { return 2 * n_sign + 2 * sum_crt + 6 * k; }
};
// Tables of one element: the multiply's g [sum_crt] and e [k][3] and the cap [k][2]. slo0 / shi0 (garbler) and
// slo / shi (evaluator) are the two sign gadgets' mod-2 output (base) labels; gate = the slot-2 stream.
void clip_mult_garble(const ClipPlan& P, const LabelBank& R, const Prg& prg, u64 stream, const comp_t* const* x0,
                      const comp_t* slo0, const comp_t* shi0, u128* g, u128* e, u128* cap, comp_t* const* out0);
void clip_mult_eval(const ClipPlan& P, const comp_t* const* x, const comp_t* slo, const comp_t* shi, const u128* g,
                    const u128* e, const u128* cap, comp_t* const* out, u64 gate);
// base labels of the wire x - q on the labels of x: x0_j + (q mod p_j) R_j (dst: k rows of 128 components)
void clip_shift_base(const ClipPlan& P, const LabelBank& R, const comp_t* const* x0, i64 q, comp_t* dst);

// ---------------------------------------------------------------------------
// ArgMax (index of the largest of K candidates; ties to the lowest index) per
// output position
//
// The max tournament (layers.h MaxTree: level l pairs slots 2q / 2q + 1, an odd
// last slot is carried) over candidates (v, i) = (value, index). Slot order is
// index order, so in a pair (a, b) the candidate a holds the lower indices.
//   d_j = v_a,j - v_b,j (free), s = [d >= 0]  (mod-2 label)
// from one exact SignMrsPlan sign of d; an approximate sign errs exactly where
// two values are close, which is where an argmax is decided, so only the exact
// sign is offered. s = 1 keeps a, also on a tie: the lowest index wins.
//   value  v_j = v_b,j + s d_j     the ReLU's mixed-modulus half gates keyed by
//          the label of s (mm.g [P], mm.e [k][3]); omitted at the root level,
//          whose value nobody reads;
//   index  level 0: both indices are public, i_j = i_b + s (i_a - i_b) mod p_j
//          is a 2-row projection Z_2 -> Z_{p_j} of s per residue (idx [k][2],
//          row = colour of s; the Clip cap's gate form, rows (TW_CAP, 0) slot j)
//          with i_b folded into the output base label;
//          later levels: e_j = i_a,j - i_b,j, i_j = i_b,j + s e_j, a second set
//          of half gates keyed by s (im.g [P], im.e [k][3]). A carried candidate
//          that has not played yet has a public index c: it is folded into the
//          base labels, e = i_a - c on the labels of i_a and c into the output
//          base, as the Clip folds its bounds.
// Hardened encoding only (the folds, and one sign label keying up to 2 k + 2
// rows). The sign, the value gates and the index gates (or the projection) of
// level l draw from PRG stream slots 20 + 3 l, 21 + 3 l, 22 + 3 l and mask with
// these streams as gates, so the two half-gate sets share no pad although both
// use rows (TW_MMG, j) / (TW_MMY, 0) (docs/SECURITY.md 2.2).
// Pair operation q of output position o at a level with `ops` operations over P
// positions is element e = q P + o; candidate slot s of position o is element
// s P + o, the layout of the (K, P) input itself. Tables under "lv<l>.": mrs
// [n_sign], mm.g, mm.e (not at the root), idx (level 0) or im.g, im.e (later).
// Entries per pair operation, n_sign = SignMrsPlan::n_tab, P = sum_j p_j:
//   level 0, not the root      n_sign + P + 3 k + 2 k
//   later level, not the root  n_sign + 2 (P + 3 k)
//   root, later level          n_sign + P + 3 k
//   root at level 0 (K = 2)    n_sign + 2 k
// (k = 7, first primes: 240, 305, 226, 161; K = 10: 2341 per output.)
struct ArgMaxPlan {
    std::vector<int> crt;
    i64 K = 2;
    i64 sum_crt = 0;
    std::vector<i64> prefix;  // mm.g / im.g offset of residue j
    SignMrsPlan sign;
    std::vector<int> ops, cnt;          // the MaxTree(K) schedule
    std::vector<std::vector<i64>> pub;  // [level][slot]: the slot's public index, -1 once it has played
    ArgMaxPlan() = default;
    ArgMaxPlan(const std::vector<int>& crt_, i64 K_);
    int k() const { return static_cast<int>(crt.size()); }
    int levels() const { return static_cast<int>(ops.size()); }
    bool root(int lv) const { return lv + 1 == levels(); }
    // table entries of one pair operation of level lv
    i64 op_entries(int lv) const {
        const i64 half = sum_crt + 3 * k();
        return sign.n_tab + (root(lv) ? 0 : half) + (lv == 0 ? 2 * k() : half);
    }
    // table entries per output position
    i64 entries() const {
        i64 n = 0;
        for (int lv = 0; lv < levels(); ++lv) n += ops[lv] * op_entries(lv);
        return n;
    }
    static i64 entries(const std::vector<int>& crt, i64 K) { return ArgMaxPlan(crt, K).entries(); }
};
// One pair operation of level lv. va / vb: the candidates' value labels; ia / ib: their index labels, unused
// (may be null) where the index is public (ia_pub / ib_pub >= 0). Tables of this operation: mrs [n_sign]; g, e
// (null at the root); idx (level 0) or ig, ie (later levels). vout is null at the root. Garbler: base labels.
void argmax_pair_garble(const ArgMaxPlan& P, int lv, const LabelBank& R, const Prg& prg, u64 s_stream, u64 v_stream,
                        u64 i_stream, const comp_t* const* va0, const comp_t* const* vb0, const comp_t* const* ia0,
                        i64 ia_pub, const comp_t* const* ib0, i64 ib_pub, u128* mrs, u128* g, u128* e, u128* idx,
                        u128* ig, u128* ie, comp_t* const* vout0, comp_t* const* iout0);
void argmax_pair_eval(const ArgMaxPlan& P, int lv, u64 s_gate, u64 v_gate, u64 i_gate, const comp_t* const* va,
                      const comp_t* const* vb, const comp_t* const* ia, const comp_t* const* ib, bool ib_pub,
                      const u128* mrs, const u128* g, const u128* e, const u128* idx, const u128* ig, const u128* ie,
                      comp_t* const* vout, comp_t* const* iout);

// ---------------------------------------------------------------------------
// Mul (product of two secret CRT tensors, or the square of one) per output
// element e
//
// Product: gen_mult_garble as it stands per residue j. r = the colour of y's
// zero label; the garbler half gate g is keyed by x (row = colour of x, tweak
// (TW_MMG, j)), the evaluator half gate e by y (row = colour of y, tweak
// (TW_GME, j)); out = E + colour(y) x - G. Gate id and PRG stream are
// stream_id(L, 1, e) of the OUTPUT element, draws per element j ascending, sk03
// then sk04. With a channel broadcast (bc = H W > 0) element e reads y[e / bc]:
// one y label keys the e rows of bc elements, each under its own gate id, so no
// two of them share a pad. Tables g [N][P], e [N][P], P = sum_j p_j.
// Square: one projection v -> v^2 mod p_j per residue (garble_proj, identity
// offset bank, tweak (TW_PROJ, j)), one fresh output label per residue drawn j
// ascending from the same stream. Table t [N][P]: half the entries, one hash
// instead of two, and no label keys two half gates.
// Hardened encoding only: without a gate tweak a label read by a Mul and by any
// other gate (a skip tensor, a broadcast y, one tensor into two Muls) would be
// hashed to the same pad (docs/SECURITY.md).
struct MulPlan {
    std::vector<int> crt;
    i64 bc = 0;  // elements per channel of a broadcast y, 0 = elementwise
    bool square = false;
    i64 sum_crt = 0;
    std::vector<i64> prefix;  // table offset of residue j
    MulPlan() = default;
    MulPlan(const std::vector<int>& crt_, i64 bc_, bool square_) : crt(crt_), bc(bc_), square(square_) {
        DASH_CHECK(bc >= 0 && !(square && bc), "mul: a square has no broadcast operand");
        for (int p : crt) {
            prefix.push_back(sum_crt);
            sum_crt += p;
        }
    }
    int k() const { return static_cast<int>(crt.size()); }
    i64 ysrc(i64 e) const { return bc ? e / bc : e; }  // y's element of output element e
    i64 ny(i64 N) const { return bc ? N / bc : N; }     // y's elements for N outputs
    i64 entries() const { return square ? sum_crt : 2 * sum_crt; }
    static i64 entries(const std::vector<int>& crt, bool square) { return MulPlan(crt, 0, square).entries(); }
};
// One output element. x0 / y0 (x / y): k label pointers; g, e (product) or t (square, passed as g; e unused): the
// element's table rows. Garbler: base labels.
void mul_garble_elem(const MulPlan& P, const LabelBank& R, const Prg& prg, u64 stream, const comp_t* const* x0,
                     const comp_t* const* y0, u128* g, u128* e, comp_t* const* out0);
void mul_eval_elem(const MulPlan& P, u64 gate, const comp_t* const* x, const comp_t* const* y, const u128* g,
                   const u128* e, comp_t* const* out);

// ---------------------------------------------------------------------------
// MatMul (wire kind 22, docs/MATMUL.md): out[i, l] = sum_t x[i, t] y[t, l], the
// contraction of two secret CRT tensors. x is M x T and y is T x N after the
// transpose flags, which only change the strides into the flat tensors:
// x[i, t] = flat_x[i xsi + t xst], y[t, l] = flat_y[t yst + l ysl].
// Per output element o = i N + l the products t = 0..T-1 are MulPlan products as
// they stand (gen_mult_garble / gen_mult_eval per residue j): product (o, t) has
// gate id and PRG stream stream_id(L, 1, o T + t) and MulPlan's draw order. The
// output zero label is the sum over t of the products' output zero labels mod
// p per component; the evaluator sums the products' output labels. One x label
// keys the g rows of N products and one y label the e rows of M, each under
// its own gate id, and the two half gates of a product differ in their tweak
// (TW_MMG / TW_GME), so a label that is both operands (x x^T) still gets two
// distinct pads. Tables g, e [M N T][P], output-major with t innermost: one
// output's rows are contiguous. Hardened encoding only, for MulPlan's reasons.
// Heads (param G, default 1): both operands are G contiguous slabs of M T and
// T N elements, head g contracts slab g of x with slab g of y, and the output
// is head-major, o = (g M + i) N + l. M, T, N and the strides stay per head; the
// gate ids, the draws and the table layout follow o as they stand, over
// G M N T products.
struct MatMulPlan {
    std::vector<int> crt;
    i64 M = 0, T = 0, N = 0;
    bool ta = false, tb = false;
    i64 G = 1;
    i64 xsi = 0, xst = 0, yst = 0, ysl = 0;
    i64 sum_crt = 0;
    std::vector<i64> prefix;  // table offset of residue j
    MatMulPlan() = default;
    MatMulPlan(const std::vector<int>& crt_, i64 M_, i64 T_, i64 N_, bool ta_, bool tb_, i64 G_ = 1)
        : crt(crt_), M(M_), T(T_), N(N_), ta(ta_), tb(tb_), G(G_) {
        DASH_CHECK(M >= 1 && T >= 1 && N >= 1 && G >= 1, "matmul: empty operand");
        DASH_CHECK(M <= (i64(1) << 36) / T && M * T <= (i64(1) << 36) / N && M * T * N <= (i64(1) << 36) / G,
                   "matmul: G M N T products do not fit the 36-bit element field of a stream id");
        xsi = ta ? 1 : T;
        xst = ta ? M : 1;
        yst = tb ? 1 : N;
        ysl = tb ? T : 1;
        for (int p : crt) {
            prefix.push_back(sum_crt);
            sum_crt += p;
        }
    }
    int k() const { return static_cast<int>(crt.size()); }
    i64 nout() const { return G * M * N; }
    i64 nx() const { return G * M * T; }
    i64 ny() const { return G * T * N; }
    // x's and y's flat element of product (o, t): the head's slab, then the strides within it
    i64 xidx(i64 o, i64 t) const { return (o / (M * N)) * (M * T) + ((o / N) % M) * xsi + t * xst; }
    i64 yidx(i64 o, i64 t) const { return (o / (M * N)) * (T * N) + t * yst + (o % N) * ysl; }
    i64 entries() const { return 2 * sum_crt * T; }                   // per output element
    static i64 entries(const std::vector<int>& crt, i64 T) { return MatMulPlan(crt, 1, T, 1, false, false).entries(); }
};
// One output element o. x0 / y0 (x / y): label pointers [t k + j] of the products' operands; g, e: the output's
// T P table rows; out0 / out: k label pointers. Garbler: base labels.
void matmul_garble_elem(const MatMulPlan& P, const LabelBank& R, const Prg& prg, u64 layer, i64 o,
                        const comp_t* const* x0, const comp_t* const* y0, u128* g, u128* e, comp_t* const* out0);
void matmul_eval_elem(const MatMulPlan& P, u64 layer, i64 o, const comp_t* const* x, const comp_t* const* y,
                      const u128* g, const u128* e, comp_t* const* out);

// ----------------------------------------------------------------------------
// LeakyRelu (wire kind 20, docs/LEAKY_RELU.md): y = 2^s x (x >= 0), n_c x (x < 0), n_c in [0, 2^s) per
// channel c = e / bc, which is n_c x + (2^s - n_c) relu(x). A public multiple and a sum of labels of one
// residue are free, so the layer garbles exactly the ReLU of its resolved sign construction (same arrays,
// layouts, PRG streams and gate ids: the tables are a ReLU's byte for byte) and then maps the labels per
// residue p: out = (n_c mod p) x + ((2^s - n_c) mod p) relu. The garbler maps the zero labels, the evaluator
// the active ones.
struct LeakyPlan {
    int s = 0;
    std::vector<i64> n;  // one slope numerator, or one per channel
    i64 bc = 0;          // elements per channel
    LeakyPlan() = default;
    LeakyPlan(i64 s_, const std::vector<i64>& n_, i64 bc_, i64 N) : s(static_cast<int>(s_)), n(n_), bc(bc_) {
        DASH_CHECK(s_ >= 1 && s_ <= 8, "leaky_relu: slope_bits outside [1, 8]");
        DASH_CHECK(!n.empty() && bc >= 1 && (n.size() == 1 || static_cast<i64>(n.size()) * bc == N),
                   "leaky_relu: slope table does not match the tensor");
        for (i64 v : n) DASH_CHECK(v >= 0 && v < (i64{1} << s), "leaky_relu: slope numerator outside [0, 2^s)");
    }
    i64 channel(i64 e) const { return n.size() == 1 ? 0 : e / bc; }
    int b(i64 ch, int p) const { return static_cast<int>(n[ch] % p); }
    int c(i64 ch, int p) const { return static_cast<int>(((i64{1} << s) - n[ch]) % p); }
    // the device tables: [channel][residue] pairs (b, c) as b | c << 8 (p <= 251)
    std::vector<uint16_t> table(const std::vector<int>& crt) const {
        std::vector<uint16_t> t(n.size() * crt.size());
        for (size_t ch = 0; ch < n.size(); ++ch)
            for (size_t j = 0; j < crt.size(); ++j)
                t[ch * crt.size() + j] = static_cast<uint16_t>(b(ch, crt[j]) | (c(ch, crt[j]) << 8));
        return t;
    }
    // out = b x + c relu per element and residue; out may alias relu
    void map(const CrtLabels& x, const CrtLabels& relu, CrtLabels& out) const {
        for (size_t j = 0; j < x.size(); ++j) {
            const int p = x[j].p, nn = x[j].n;
            for (i64 e = 0; e < x[j].N; ++e) {
                const i64 ch = channel(e);
                const int bb = b(ch, p), cc = c(ch, p);
                const comp_t* xe = x[j].at(e);
                const comp_t* re = relu[j].at(e);
                comp_t* oe = out[j].at(e);
                for (int i = 0; i < nn; ++i) oe[i] = static_cast<comp_t>((bb * xe[i] + cc * re[i]) % p);
            }
        }
    }
};

// ----------------------------------------------------------------------------
// PiecewiseLinear (wire kind 21, docs/PWL.md): y = V + A_0 (x - T_1) + sum_i D_i relu(x - T_i) with m <= 8
// breakpoints T_1 < ... < T_m, slope numerators A_0 .. A_m over 2^s and D_i = A_i - A_(i-1); breakpoints with
// D_i = 0 are dropped. Per kept breakpoint i (in order, i = 0 .. m-1): one sign s_i = [x - T_i >= 0] of the
// layer's resolved sign construction and the ReLU's mixed-modulus half gates keyed by s_i, both on the evaluator's
// labels of x: T_i is folded into the garbler's base labels (x0_j + T_i R_j is the base of the wire x - T_i, as
// the Clip folds its bounds). The output is the free combination per residue p
//   out = (A_0 mod p) x + sum_i (D_i mod p) t_i,   t_i = relu(x - T_i),
// of zero labels on the garbler (shifted bases, and the constant V - A_0 T_1 folded in: out0 -= (V - A_0 T_1) R)
// and of active labels on the evaluator. Arrays under "b<i>.": mrs or s.approx / s.cast2 / s.sign, mm.g [P],
// mm.e [k][3]. PRG stream slot of sign i: 1 + 2i, of multiply i: 2 + 2i (at most 16 < ArgMax's 20): distinct
// slots give distinct gate ids, so no two breakpoints share a pad although they read the same labels.
// Hardened encoding only. Entries per element: m (n_sign + P + 3k).
struct PwlPlan {
    static constexpr int kMaxBreaks = 8;
    std::vector<int> crt;
    int s = 0;
    std::vector<i64> T, D;  // the kept breakpoints and their slope steps (D != 0)
    i64 A0 = 0, C = 0;      // first slope numerator; the constant V - A_0 T_1 (T_1: the first breakpoint given)
    i64 sum_crt = 0;
    std::vector<i64> prefix;  // mm.g offset of residue j
    PwlPlan() = default;
    PwlPlan(const std::vector<int>& crt_, i64 s_, const std::vector<i64>& T_, const std::vector<i64>& A_, i64 V)
        : crt(crt_), s(static_cast<int>(s_)) {
        DASH_CHECK(s_ >= 1 && s_ <= 8, "pwl: slope_bits outside [1, 8]");
        DASH_CHECK(!T_.empty() && static_cast<int>(T_.size()) <= kMaxBreaks && A_.size() == T_.size() + 1,
                   "pwl: between 1 and 8 breakpoints and one more slope");
        for (size_t i = 0; i + 1 < T_.size(); ++i) DASH_CHECK(T_[i] < T_[i + 1], "pwl: breakpoints must increase");
        for (i64 a : A_) DASH_CHECK(a >= -(i64{2} << s) && a <= (i64{2} << s), "pwl: slope numerator beyond 2 * 2^s");
        for (size_t i = 0; i < T_.size(); ++i)
            if (A_[i + 1] != A_[i]) {
                T.push_back(T_[i]);
                D.push_back(A_[i + 1] - A_[i]);
            }
        DASH_CHECK(!T.empty(), "pwl: no breakpoint left (every slope step is 0)");
        A0 = A_[0];
        C = V - A0 * T_[0];
        for (int p : crt) {
            prefix.push_back(sum_crt);
            sum_crt += p;
        }
    }
    int k() const { return static_cast<int>(crt.size()); }
    int m() const { return static_cast<int>(T.size()); }
    static int sign_slot(int i) { return 1 + 2 * i; }
    static int mult_slot(int i) { return 2 + 2 * i; }
    static std::string prefix_of(int i) { return "b" + std::to_string(i) + "."; }
    i64 entries(i64 n_sign) const { return m() * (n_sign + sum_crt + 3 * k()); }
    int a0(int p) const { return static_cast<int>(((A0 % p) + p) % p); }
    int d(int i, int p) const { return static_cast<int>(((D[i] % p) + p) % p); }
    int c(int p) const { return static_cast<int>(((C % p) + p) % p); }
    // the device table [residue][m + 1]: A_0 mod p, then D_i mod p
    std::vector<uint8_t> table() const {
        std::vector<uint8_t> t;
        for (int p : crt) {
            t.push_back(static_cast<uint8_t>(a0(p)));
            for (int i = 0; i < m(); ++i) t.push_back(static_cast<uint8_t>(d(i, p)));
        }
        return t;
    }
};
// One element's table rows per kept breakpoint: the exact sign's row (mrs) or the approximate sign's three
// (approx, cast2, sign), and the multiply's g [sum_crt] and e [k][3].
struct PwlRows {
    u128* mrs[PwlPlan::kMaxBreaks] = {};
    u128* approx[PwlPlan::kMaxBreaks] = {};
    u128* cast2[PwlPlan::kMaxBreaks] = {};
    u128* sign[PwlPlan::kMaxBreaks] = {};
    u128* g[PwlPlan::kMaxBreaks] = {};
    u128* e[PwlPlan::kMaxBreaks] = {};
};
// sp_m: the exact sign (rows mrs) or, when null, sp_a: the approximate fused sign. stream(slot) is the PRG stream
// / gate id of the element for a slot (stream_id(L, slot, e)). x0 / out0: base labels; x / out: active labels.
void pwl_garble_elem(const PwlPlan& P, const SignPlan* sp_a, const SignMrsPlan* sp_m, const LabelBank& R,
                     const LabelBank& Z, const Prg& prg, const u64* sign_streams, const u64* mult_streams,
                     const comp_t* const* x0, const PwlRows& t, comp_t* const* out0);
void pwl_eval_elem(const PwlPlan& P, const SignPlan* sp_a, const SignMrsPlan* sp_m, const LabelBank& Z,
                   const u64* sign_gates, const u64* mult_gates, const comp_t* const* x, const PwlRows& t,
                   comp_t* const* out);

}  // namespace dash
