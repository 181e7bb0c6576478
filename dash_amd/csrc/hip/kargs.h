// Kernel argument structs shared by the HIP kernels and the host runtime.
#pragma once

#include <stdint.h>

#include "dev.h"

namespace dash {
namespace dev {

constexpr int kMaxRes = 16;   // max CRT residues on the GPU path
constexpr int kMaxMrs = 16;
constexpr int kMaxOut = 16;

// Label components of activations are stored as bytes: every modulus of the
// GPU path is < 256 (CRT primes, ReDash bases <= 173, power-of-two moduli <=
// 128), so each streaming kernel moves half the bytes of int16 labels. Tables,
// constant labels and the host format stay int16.
typedef uint8_t act_t;
constexpr int kActMaxModulus = 255;

// Residue-major activation description: act[j] -> act_t [B][n_j][N]
struct Act {
    act_t* p[kMaxRes];
    int64_t N;  // elements per GC
};

struct CrtInfo {
    int k;
    int p[kMaxRes];
    int n[kMaxRes];
    int prefix[kMaxRes];
    int sum;
};

// Garbler-side input encoding on the device (k_encode_in), per slot s:
// out_j[s][c][e] = W0_j[s][c][e] + (x[s][e] mod p_j) R_j[s][c] mod p_j
struct EncIn {
    int k;
    int p[kMaxRes];
    int n[kMaxRes];
    const act_t* w0[kMaxRes];  // [n_j][N] component-major input base labels
    const act_t* r[kMaxRes];   // [n_j] the offset R_{p_j}
    act_t* out[kMaxRes];       // [n_j][N] an evaluator slot's input activations (slot s + 1 follows n_j N later)
    int64_t wstride;           // bytes between the encoder slots' W0 / R blocks (grid z = slot)
    // set by launch_encode_in: component prefix of residue j (pre[k] = total) and 1 / p_j
    int pre[kMaxRes + 1];
    float inv[kMaxRes];
};

struct SignArgs {
    CrtInfo crt;
    int t;
    int mrs[kMaxMrs];
    int nout;
    int out_mod[kMaxOut];
    int64_t N;           // elements
    int B;
    int64_t n_approx, n_cast, n_sign;  // table entries per element
    const u128* approx;  // [B][N][n_approx]
    const u128* cast1;   // [B][N][n_cast]
    const u128* cast2;
    const u128* sign;    // [B][N][n_sign]
    u128* mrsP;          // [B][k][t][N] compressed approx outputs
    u128* hx;            // [B][k][N] H(compress(x_j)) (ReLU reuse) - may be null
    uint16_t* colx;      // [B][k][N]
    u128* outP;          // [B][nout][N] compressed sign outputs
    u128* hs;            // [B][N] H(compress(sign mod 2)) when relu != 0
    uint8_t* cs;         // [B][N]
    const u128* zc;      // [B][zc_stride] compressed zero labels, indexed by modulus
    const uint16_t* zcol;  // [B][zc_stride] zero-label colors
    int zc_stride;
    int relu;            // also produce hs / cs for the ReLU multiply
    int16_t* csum;       // [B][t][kCsumComps][N] per-digit sums of the k cast labels (phase B1)
    int64_t c1off[kMaxMrs];  // offset of digit d's block ((k+1) m_d entries) in a cast1 row
    int fused;           // SignPlan::fused: approx outputs are already cast, carries come out cast (no cast1)
    // hardened encoding (dev.h hard_block): hx holds the ReLU garbler half gates' pads, ys the sign label's
    // evaluator-half pads [B][ny][N] (slots 0..k-1 the residues' entries, k.. the packed mini lanes)
    int hard;
    uint64_t sgate0, mgate0;  // gate bases of the sign gadget / the mixed-mult gadget (dev.h gate_base)
    int ny;
    u128* ys;
};
constexpr int kCsumComps = 64;

// LeakyRelu epilogue of the ReLU multiply (gadgets.h LeakyPlan): t[channel][k] = b | c << 8 with b = n_c mod p_j,
// c = (2^s - n_c) mod p_j; channel = e / bc (a scalar slope: one channel, bc = N)
struct LeakyTab {
    const uint16_t* t;
    uint32_t bc;
};

// PiecewiseLinear multiply (gadgets.h PwlPlan): the m kept breakpoints' half gates in one pass over the label of
// x. kx / colx: the compressed labels and colours of x (k_label_key; every breakpoint's (TW_MMG, j) pad is
// derived from kx under its own gate). key[i]: breakpoint i's sign label [B][N]; gtab / etab: its b<i>.mm.g /
// b<i>.mm.e; mgate0[i] = gate_base(L, 2 + 2i). fac[residue][m + 1] = A_0 mod p, then D_i mod p.
constexpr int kPwlMax = 8;
struct PwlArgs {
    CrtInfo crt;
    int64_t N;
    int m;
    const u128* kx;
    const uint16_t* colx;
    const u128* key[kPwlMax];
    const u128* gtab[kPwlMax];
    const u128* etab[kPwlMax];
    uint64_t mgate0[kPwlMax];
    const uint8_t* fac;
};

struct RescaleArgs {
    CrtInfo crt;
    int64_t N;
    int fi, s;
    int add_up;
    int active[kMaxRes];   // 1 if residue is processed by this factor
    int aidx[kMaxRes];     // index among active residues (table offset / s)
    int inv[kMaxRes];      // s^-1 mod p_j
    int64_t n_trans, off;  // entries per element, offset of this factor
    const u128* trans;     // [B][N][n_trans]
    const u128* h0;
    const uint16_t* col0;
    const int16_t* up;     // [B][sum n] per-GC upshift labels (residue-concatenated)
    const int16_t* zero;   // [B][sum n] zero labels of the CRT moduli
    int lab_stride;        // sum_j n_j
    int lab_off[kMaxRes];  // offset of residue j inside up/zero rows
    int hard;              // hardened encoding: trans pads (TW_TRANS, factor) instead of H
    uint64_t gate0;
    int factor;            // index of this factor (the trans row's tweak)
};

// Single-shot mixed-radix rescale (gadgets.h RescaleMrsPlan)
struct MrsArgs {
    CrtInfo crt;
    int T;                         // 2^(l+1): modulus of the x_u mod 2S label (power of two)
    int64_t N, n_tab;
    const u128* tab;               // [B][N][n_tab]
    int64_t dig_off[kMaxRes];      // digit i rows: [color][k - i]
    int64_t fin_off;               // final rows: [color][k]
    int sinv[kMaxRes];             // S^-1 mod p_j (j >= 1)
    u128 hmask;                    // top bit of every log2(T)-bit field (packed mod-T additions)
    u128* pf;                      // [B][k][N] final payloads (chain -> output kernel)
    u128* ps;                      // [B][k(k-1)/2][N] digit payloads for later positions (chain scratch)
    int mode;                      // 0: rescale (position i = residue i, T accumulator, final row -> pf)
                                   // 1: sign (position i = residue (i + 1) mod k; the last key is sign01 -> hs, cs)
                                   // 2: rescale in mode 1's order, the mod-2 key is also the next ReLU's sign
    u128* hs;                      // modes 1, 2: [B][N] hash of the sign label
    uint8_t* cs;                   // modes 1, 2: [B][N] its color
    u128* hx;                      // mode 2: [B][k][N] H(compress(Y_j)) of the outputs (the next ReLU's keys)
    uint16_t* colx;                // mode 2: [B][k][N] their colors
    // hardened encoding (the only one of the mixed-radix constructions): row pads instead of H
    uint64_t gate0;   // this gadget's gate base (rescale: stream slot 30, sign: slot 1)
    uint64_t rgate0;  // modes 1, 2: the ReLU mixed-mult gadget's gate base (its y-row / g-row pads)
    int ny;           // y-row pad slots per element (k entries + packed minis)
    u128* ys;         // modes 1, 2: [B][ny][N] the sign label's y-row pads
    u128* ks;         // mode 1, a Clip's sign: [B][N] the sign label itself (with ny = 0: no y-row pads); else null
    int qpack;        // k_mrs_chain_q: bit 0 four digits per quad reduction (moduli <= 63); >> 1: positions
                      // I < that value take chunk-split keys
    int cmod;         // joint output kernels (k_rescale_*_out_t): 1 takes the constant-modulus walks (launch.h
                      // const_mod_on; the launcher sets it at every launch)
};

// Clip multiply (gadgets.h ClipPlan): the two sign labels, the half gates' tables and the cap rows
struct ClipArgs {
    CrtInfo crt;
    int64_t N;
    const u128* hx;        // [B][k][N] pads of x_j's garbler half gate row (TW_MMG, j), gate mgate0
    const uint16_t* colx;  // [B][k][N]
    const u128* klo;       // [B][N] compressed sign label s_lo = [x >= q_lo]
    const u128* khi;       // [B][N] compressed sign label s_hi = [x >= q_hi]
    const u128* gtab;      // [B][N][sum]
    const u128* etab;      // [B][N][k][3]
    const u128* cap;       // [B][N][k][2]
    uint64_t mgate0;       // gate base of the multiply (stream slot 2): rows (TW_MMY, 0) of u, (TW_CAP, 0) of s_hi
};

// One level of an ArgMax (gadgets.h ArgMaxPlan): `ops` pair operations over `cnt` candidate slots at each of P
// positions. Slot s of position o is element s P + o of the candidate buffers, pair operation q is element
// e = q P + o of the per-operation arrays (N = ops P) and of the next level's slot q.
struct ArgMaxArgs {
    CrtInfo crt;
    int64_t P;
    int ops, cnt, cnt1;    // cnt1 = slots of the next level (ops, + 1 with a carried slot)
    int pubq;              // the pair operation whose b candidate has a public index (the last one), else -1
    int carry_idx;         // the carried slot (cnt odd) has index labels to copy (it has played)
    const u128* ks;        // [B][N] compressed sign labels s = [v_a >= v_b]
    const u128* hx;        // [B][k][N] value gates: pads of d_j's garbler half gate row (TW_MMG, j), gate vgate0
    const uint16_t* colx;  // [B][k][N]
    const u128* hi;        // the same of the index difference e_j under igate0 (levels >= 1)
    const uint16_t* coli;
    const u128* gtab;      // mm.g [B][N][sum]     (not at the root)
    const u128* etab;      // mm.e [B][N][k][3]
    const u128* itab;      // idx  [B][N][k][2]    (level 0)
    const u128* igtab;     // im.g [B][N][sum]     (levels >= 1)
    const u128* ietab;     // im.e [B][N][k][3]
    uint64_t vgate0, igate0;  // gate bases of the value gates and of the index gates / projection
};

struct BEArgs {
    int E, nonext;
    int swapped[kMaxRes];    // moduli in MRS order
    int src[kMaxRes];        // residue index of position i
    int inv[kMaxRes][kMaxRes];  // inv_partial[i][j]
    int nextra;
    int extra_pos[kMaxRes];  // position (in swapped order) of extra residue x
    int extra_res[kMaxRes];  // residue index of extra x
    int invv[kMaxRes];
    int64_t N, n_tab;
    const u128* tab;         // [B][N][n_tab]
    int16_t* work;
    int hard;
    uint64_t gate0;
};

struct ProjArgs {
    int k;
    int pin[kMaxRes], pout[kMaxRes];
    const u128* tab[kMaxRes];  // [B][N][pin_j]
    int64_t N;
    int hard;
    uint64_t gate0;
};

struct MultArgs {
    CrtInfo crt;
    int64_t No;  // outputs per GC
    int q;       // 0 = same-modulus multiply, else mixed with modulus q
    const u128* t;  // [B][No][sum]   (mixed only)
    const u128* g;  // [B][No][sum]
    const u128* e;  // same: [B][No][sum]; mixed: [B][No][k][q+1]
    int hard;
    uint64_t gate0;
};

// A Mul layer (gadgets.h MulPlan; hardened only): out[e] = x[e] * y[bc ? e / bc : e] over N outputs per GC, or
// the square x[e]^2 (g = the table t, e unused). y is a saved output of Ny elements per GC, read for its
// compressed label and colour only.
struct MulArgs {
    CrtInfo crt;
    int64_t N, Ny;
    int64_t bc;     // elements per channel of a broadcast y, 0 = elementwise
    const u128* g;  // [B][N][sum] rows (TW_MMG, j) keyed by x; the square's rows (TW_PROJ, j)
    const u128* e;  // [B][N][sum] rows (TW_GME, j) keyed by y
    uint64_t gate0;
};

// A MatMul layer (gadgets.h MatMulPlan; hardened only): out[i N + l] = sum_t x[i xsi + t xst] * y[t yst + l ysl]
// over M N outputs per GC. Neither operand's label is read by the multiply: kx / ky hold their compressed labels
// and cx / cy their colours, [B][k][M T] and [B][k][T N], written once per run by the key pre-pass
// (launch_label_key). The digits of x come from kx itself. With G > 1 heads the operands are G slabs of M T and
// T N elements and the outputs G slabs of M N, head-major: every array above has G times the elements, and M, T, N
// and the strides stay per head.
struct MatMulArgs {
    CrtInfo crt;
    int64_t M, T, N;
    int64_t G;  // heads, >= 1
    int64_t xsi, xst, yst, ysl;  // the transposes, as strides
    const u128* g;               // [B][M N T][sum] rows (TW_MMG, j) keyed by x, t innermost
    const u128* e;               // [B][M N T][sum] rows (TW_GME, j) keyed by y
    const u128 *kx, *ky;
    const uint16_t *cx, *cy;
    uint64_t gate0;
    int lds_n;    // the widest label of an odd residue: rows of the accumulator image (and of the blocked form's digits)
    int blocked;  // the planner's pick: k_matmul_b (matmul.blocked) instead of k_matmul (matmul.lane)
};
// The blocked form's tile: kMmI x kMmL outputs per block, kMmTC products of t per staged chunk
constexpr int kMmI = 16, kMmL = 16, kMmTC = 16;

}  // namespace dev
}  // namespace dash
