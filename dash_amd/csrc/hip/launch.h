// Host-side launchers for the HIP kernels (implemented in kernels_*.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "kargs.h"

namespace dash {
namespace dev {

// Launch planning (launch_plan.hip). num_cus() is the CU count the pickers of the gadget launches compare a
// launch with: the device's count, or the override a test set with set_planning_cus (n = 0 restores the device's
// value; nothing else sets it, no environment variable either). It changes only which kernel form, block size and
// grid a picker chooses, never where the work runs, and none of the pickers' correctness preconditions.
int num_cus();
void set_planning_cus(int n);
int planning_cus_override();  // 0: none
// Joint rescale + ReLU: whether the planner defers the rescale's outputs to the ReLU's fused output kernel
// (launch_rescale_relu_out) instead of the output-hash and ReLU-multiply kernels. Mode -1 (auto) follows
// joint_fuse_pick, 0 / 1 force it off / on; the DASH_JOINT_FUSE environment value is the initial mode. Like the
// planning count, an evaluator reads it when it plans: set it before building the evaluator. (Defined beside
// launch_rescale_relu_out in kernels_gadget.hip: launch_plan.hip reads no environment.)
// joint_fuse_pick is the pure host rule: batches of at most 2 GCs (latency), and staged shapes (stage_ok at 256
// lanes) of at least joint_fuse_min_elems() elements over the batch. The threshold is an absolute element
// count: it does not follow the planning CU count.
int64_t joint_fuse_min_elems();
int joint_fuse_mode();
void set_joint_fuse(int mode);
bool joint_fuse_pick(int64_t N, int B);
bool joint_fuse(int64_t N, int B);  // the mode applied to the rule
// The same for a joint Clip behind the rescale (launch_rescale_clip_out): the mode forces it, the auto rule
// clip_fuse_pick is the Clip's own (not joint_fuse_pick's threshold).
// A joint LeakyRelu defers where joint_fuse_pick's throughput branch does (batches of at least 3 GCs, the same
// element threshold); the mode forces it as it does the ReLU's.
bool leaky_fuse(int64_t N, int B);
bool clip_fuse_pick(int64_t N, int B);
bool clip_fuse(int64_t N, int B);
// Constant-modulus kernel forms (dev.h ModK). Mode 0: none, the run-time-modulus forms of the same build (A/B on one
// device); 1: the joint output kernels' per-residue walks; 2: also the staged chain of a first-primes base of 7
// residues. The DASH_CONST_MOD environment value is the initial mode, kConstModDefault without one. The chain's
// form is opt-in: it spills more than the generic chain and was not faster (profiles/ab/const_mod/README.md). The
// mode is read at every host-side launch; an evaluator's launches are frozen when its graph is captured, so set it
// before the evaluator's first run. Results are bit-identical in every mode. const_mod_launches counts the
// host-side launches that took a constant form (chain: the staged chain, else an output kernel): the launch log's
// lines do not tell the forms apart. (Defined in kernels_gadget.hip.)
constexpr int kConstModDefault = 1;
int const_mod_mode();
void set_const_mod(int mode);
inline bool const_mod_on() { return const_mod_mode() >= 1; }
inline bool const_mod_chain() { return const_mod_mode() >= 2; }
void const_mod_count(bool chain);
long const_mod_launches(bool chain);
// The staged chain's rule (pure host arithmetic): the base is the first 7 primes, the one K whose constant-modulus
// chain is compiled (mrs_chain.h kChainFpK). The joint output kernels need no rule: they dispatch per residue.
constexpr int kChainFpK = 7;  // the headline base; another K costs its chain unit's build time again (docs/BUILD.md)
inline bool chain_const_mod_pick(const int* p, int k) {
    if (k != kChainFpK) return false;
    for (int r = 0; r < k; ++r)
        if (p[r] != static_cast<int>(kFirstPrimes[r])) return false;
    return true;
}
// Launch log: off by default (one relaxed load per host-side launch, nothing under graph replay, where no picker
// runs). When on, every picker appends the form it launched as "<form> grid=(x,y,z) block=n".
extern std::atomic<bool> g_launch_log_on;
inline bool launch_log_on() { return g_launch_log_on.load(std::memory_order_relaxed); }
void launch_log_enable(bool on);
void launch_log_add(const std::string& form, dim3 grid, dim3 block);
std::vector<std::string> launch_log_take();


void launch_sign_approx(const SignArgs& a, const Act& x, const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_sign_chain(const SignArgs& a, int maxn, const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_unpack(const u128* P, int nres, const Act& out, const CrtInfo& mods, const ModC* mc, int64_t N, int B,
                   hipStream_t st);
void launch_clip_hash(const ClipArgs& a, u128* hx, uint16_t* colx, const Act& x, int B, const ModC* mc,
                      const AesGlobals& g, hipStream_t st);
void launch_clip_sign_mrs(const MrsArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_clip_mult(const ClipArgs& a, const Act& x, const Act& y, int B, const ModC* mc, hipStream_t st);
void launch_argmax_diff(const Act& v, const Act& d, int64_t P, int ops, int cnt, int pubq, const CrtInfo& crt, int B,
                        hipStream_t st);
void launch_argmax_hash(const Act& d, const CrtInfo& crt, int64_t N, u128* hx, uint16_t* colx, uint64_t gate0, int B,
                        const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_argmax_mult(const ArgMaxArgs& a, bool val, bool l0, const Act& v, const Act& d, const Act& i, const Act& ed,
                        const Act& nv, const Act& ni, int B, const ModC* mc, hipStream_t st);
// PiecewiseLinear (gadgets.h PwlPlan): the compressed labels / colours of x (k_label_key), and all kept
// breakpoints' half gates plus the linear combination in one pass (k_pwl_mult / k_pwl_mult_s, mult_grid's picker;
// log names pwl_mult.lane / pwl_mult.staged). The sign launches between the two are the Clip's.
void launch_pwl_key(const PwlArgs& a, u128* kx, uint16_t* colx, const Act& x, int B, const ModC* mc, hipStream_t st);
void launch_pwl_mult(const PwlArgs& a, const Act& x, const Act& y, int B, const ModC* mc, hipStream_t st);
// LeakyRelu: the ReLU multiply with the leaky epilogue (k_leaky_mult / k_leaky_mult_s, mult_grid's picker), and
// the deferred outputs of a joint rescale with a LeakyRelu behind it (k_rescale_leaky_out_t where
// launch_rescale_relu_out takes its throughput form; elsewhere the output-hash kernel and the leaky multiply)
void launch_leaky_mult(const SignArgs& a, const LeakyTab& lk, const Act& x, const Act& y, const u128* gtab,
                       const u128* etab, const ModC* mc, hipStream_t st);
void launch_leaky_mrs(const MrsArgs& a, const SignArgs& sa, const LeakyTab& lk, const Act& x, const Act& y,
                      const u128* gtab, const u128* etab, int B, const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_rescale_leaky_out(const MrsArgs& a, const SignArgs& sa, const LeakyTab& lk, const Act& x, const Act& y,
                              const u128* gtab, const u128* etab, int B, const ModC* mc, const AesGlobals& g,
                              hipStream_t st);
void launch_relu_mult(const SignArgs& a, const Act& x, const Act& y, const u128* gtab, const u128* etab,
                      const ModC* mc, hipStream_t st);
void launch_rescale_hash(const Act& x, int fi, int s, const int16_t* up, int up_stride, int add_up, int64_t N, int B,
                         u128* h0, uint16_t* col0, const ModC* mc, const AesGlobals& g, hipStream_t st, int hard = 0);
void launch_rescale_update(const RescaleArgs& a, const Act& x, int B, const ModC* mc, hipStream_t st);
void launch_rescale_post(const Act& x, const CrtInfo& crt, int64_t N, int B, const u128* signP, const int16_t* down,
                         int lab_stride, const int* lab_off, const ModC* mc, hipStream_t st);
void launch_rescale_hash_sign(const u128* signP, const u128* du, int64_t N, int B, u128* h0, uint16_t* col0,
                              const AesGlobals& g, hipStream_t st);
void launch_rescale_update_approx(const RescaleArgs& r, const SignArgs& a, const Act& x, const int16_t* delta,
                                  const u128* zh, int B, const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_rescale_mrs(const MrsArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g, hipStream_t st,
                        bool chain_only = false);
void launch_rescale_mrs_out(const MrsArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g,
                            hipStream_t st);
// mixed-radix chain of K residues (mrs_chain.h; instantiated per K in kernels_mrs_*.hip)
template <int K>
void launch_mrs_chain_k(const MrsArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_rescale_relu_out(const MrsArgs& a, const SignArgs& sa, const Act& x, const Act& y, const u128* gtab,
                             const u128* etab, int B, const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_rescale_clip_out(const MrsArgs& a, const ClipArgs& ca, const Act& x, const Act& y, int B, const ModC* mc,
                             const AesGlobals& g, hipStream_t st);
void launch_relu_joint(const SignArgs& sa, const Act& x, const Act& y, const u128* gtab, const u128* etab, int B,
                       const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_relu_mrs(const MrsArgs& a, const SignArgs& sa, const Act& x, const Act& y, const u128* gtab,
                     const u128* etab, int B, const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_base_ext(const BEArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g, hipStream_t st);
void launch_proj(const ProjArgs& a, const Act& x, const Act& y, int B, const ModC* mc, const AesGlobals& g,
                 hipStream_t st);
// Mul layer: x * ys (ys = the saved operand) or, with square, x^2. Logs "mul.lane" / "mul.staged" (mult_grid's
// pick) or "mul.sq".
void launch_mul(const MulArgs& a, bool square, const Act& x, const Act& ys, const Act& y, int B, const ModC* mc,
                hipStream_t st);
// MatMul layer (kernels_matmul.hip): the compressed labels and colours of an operand's N elements, once per run
// (k_label_key, [B][k][N]), and the contraction itself, which reads only those. Logs "matmul.lane" or
// "matmul.blocked" (MatMulArgs::blocked, the planner's pick).
void launch_label_key(const CrtInfo& crt, int64_t N, u128* kx, uint16_t* colx, const Act& x, int B, const ModC* mc,
                      hipStream_t st);
void launch_matmul(const MatMulArgs& a, const Act& y, int B, const ModC* mc, hipStream_t st);
void launch_mult(const MultArgs& a, const Act& x, const Act& y, int B, const ModC* mc, const AesGlobals& g,
                 hipStream_t st);

// label kernels (kernels_label.hip)
void launch_copy_gather(const Act& in, int64_t Nin, const Act& out, int64_t Nout, const int64_t* idx,
                        const CrtInfo& crt, int B, hipStream_t st);
// Gather layer: the dword form (k_gather4, idx4 = the int32 map padded to a multiple of four; needs Nout % 4 == 0 and
// 4-byte aligned out.p[j]) or, with idx4 null, the byte form (launch_copy_gather on the int64 map idx8). Logs
// "gather.dword" / "gather.byte".
void launch_gather(const Act& in, int64_t Nin, const Act& out, int64_t Nout, const int32_t* idx4, const int64_t* idx8,
                   const CrtInfo& crt, int B, hipStream_t st);
// Bilinear layer (layers.h BilinearGeom): the separable two-tap label stencil. rows / cols: the taps (i0, i1) per
// output row / column; wrow / wcol: per residue the tap weights reduced mod p_j, w0 | w1 << 8 ([k][OH] and
// [k][OWp]); cols and wcol are padded to OWp = OW rounded up to a multiple of 4, so that the dword form's vector
// loads stay aligned and in bounds; mq[j] = floor(2^32 / p_j) (dev.h div32_q). Every modulus is at most
// kActMaxModulus: four products of three bytes fit the int32 accumulator.
struct BilinearArgs {
    int C, H, W, OH, OW, OWp;
    const int2* rows;
    const int2* cols;
    const uint16_t* wrow;
    const uint16_t* wcol;
    uint32_t mq[kMaxRes];
};
// The host side of those tables, for the caller to put into device memory (the evaluator's planner and the GPU
// garbler own their uploads); sets every field of `a` but the four pointers.
struct BilinearTables {
    std::vector<int2> rows, cols;
    std::vector<uint16_t> wrow, wcol;
};
template <class Geom>  // layers.h BilinearGeom (validated: taps in range, weights in [0, 2^b])
BilinearTables bilinear_tables(BilinearArgs& a, const Geom& G, const int* mods, int k) {
    a.C = static_cast<int>(G.C); a.H = static_cast<int>(G.H); a.W = static_cast<int>(G.W);
    a.OH = static_cast<int>(G.OH); a.OW = static_cast<int>(G.OW);
    a.OWp = (a.OW + 3) / 4 * 4;
    BilinearTables t;
    t.rows.resize(static_cast<size_t>(a.OH));
    t.cols.assign(static_cast<size_t>(a.OWp), make_int2(0, 0));
    t.wrow.resize(static_cast<size_t>(k) * a.OH);
    t.wcol.assign(static_cast<size_t>(k) * a.OWp, 0);
    for (int oy = 0; oy < a.OH; ++oy)
        t.rows[oy] = make_int2(static_cast<int>((*G.y0)[oy]), static_cast<int>((*G.y1)[oy]));
    for (int ox = 0; ox < a.OW; ++ox)
        t.cols[ox] = make_int2(static_cast<int>((*G.x0)[ox]), static_cast<int>((*G.x1)[ox]));
    for (int j = 0; j < k; ++j) {
        const int p = mods[j];
        a.mq[j] = static_cast<uint32_t>((uint64_t(1) << 32) / static_cast<uint64_t>(p));
        for (int oy = 0; oy < a.OH; ++oy)
            t.wrow[static_cast<size_t>(j) * a.OH + oy] = static_cast<uint16_t>(G.wy(oy, 0, p) | G.wy(oy, 1, p) << 8);
        for (int ox = 0; ox < a.OW; ++ox)
            t.wcol[static_cast<size_t>(j) * a.OWp + ox] = static_cast<uint16_t>(G.wx(ox, 0, p) | G.wx(ox, 1, p) << 8);
    }
    return t;
}
// dword: k_bilinear4, a lane owns four consecutive ox of one output row (needs OW % 4 == 0 and 4-byte aligned
// out.p[j]); else k_bilinear, one output per lane. Logs "bilinear.dword" / "bilinear.byte".
void launch_bilinear(const BilinearArgs& g, bool dword, const Act& in, const Act& out, const CrtInfo& crt, int B,
                     hipStream_t st);
void launch_pair_diff(const Act& v, int64_t Nv, const Act& d, int64_t Nout, int ops, int cnt, const CrtInfo& crt, int B,
                      hipStream_t st);
void launch_pair_add(const Act& v, int64_t Nv, const Act& r, const Act& nv, int64_t Nout, int ops, int cnt, int cnt1,
                     const CrtInfo& crt, int B, hipStream_t st);
void launch_add(const Act& x, const Act& y, int64_t N, const CrtInfo& crt, int B, hipStream_t st);
void launch_window_sum(const Act& in, int64_t Nin, const Act& out, int64_t Nout, const int64_t* idx, int K,
                       const CrtInfo& crt, int B, hipStream_t st);
// padded / ceil-mode sum pool straight from the geometry (no index table; out-of-image taps are skipped)
struct PoolArgs {
    int C, H, W, kh, kw, sh, sw, ph, pw, OH, OW;
};
void launch_pool_sum(const Act& in, const Act& out, const PoolArgs& g, const CrtInfo& crt, int B, hipStream_t st);
// one concat operand: rows of Ns elements into rows of Nout elements at element offset off
void launch_concat_copy(const Act& src, int64_t Ns, const Act& out, int64_t Nout, int64_t off, const CrtInfo& crt,
                        int B, hipStream_t st);
void launch_aes_bench(u128* out, int blocks, int iters, const AesGlobals& g, hipStream_t st);
void launch_aes_test(const u128* in, u128* out, int64_t n, const AesGlobals& g, hipStream_t st);
void launch_hard_test(const u128* key, const uint64_t* gate, const uint32_t* sub, const uint32_t* blk, u128* out,
                      int64_t n, hipStream_t st);
// dev.h ModK<q>'s helpers on N chunk remainders r (k_modk_test): kModkTestRow zero-initialised words per element
constexpr int kModkTestRow = 64;
void launch_modk_test(int q, const uint32_t* r, int64_t N, uint32_t* out, hipStream_t st);
void launch_codec_test(const int16_t* labels, int64_t N, int q, const ModC* mc, u128* comp, int16_t* decomp,
                       hipStream_t st);

// linear layers (kernels_gemm.hip)
struct DenseArgs {
    CrtInfo crt;
    int64_t K, O;                  // in / out features
    const int16_t* w[kMaxRes];     // [K][O] weights mod p_j (or int8 packs for MFMA)
    const int32_t* zc[kMaxRes];    // [O] zero-weight counts
    const int16_t* bias[kMaxRes];  // [B][O][n_j]
    const int16_t* zero;           // [B][lab_stride]
    int lab_stride;
    int lab_off[kMaxRes];
    const int32_t* src;            // [K] input remap (channel_tf) or null
    // MFMA path (all p <= 255): centered int8 weights [O][Kpad] with the channel_tf remap folded into the
    // column order (w8[o][src(i)] = w[o][i]), zero-padded to Kpad = 64 * ceil(K / 64); null: VALU kernel
    const int8_t* w8[kMaxRes];
    int Kpad;
};
void launch_dense(const DenseArgs& a, const Act& x, const Act& y, int B, hipStream_t st);
// builds the process-wide (residue, component) lookup the VALU dense / conv kernels index blocks with, outside
// any stream capture (HipEvaluator construction calls it)
void prepare_zmap(const CrtInfo& crt);

struct ConvArgs {
    CrtInfo crt;
    int C, H, W, F, kh, kw, sh, sw, ph, pw, OH, OW;
    // dilation: tap (dy, dx) reads input (oy sh - ph + dy dh, ox sw - pw + dx dw). Honoured by the dilated kernel
    // forms only (launch_conv picks them by conv_dilated); the plain forms compile with dh = dw = 1
    int dh = 1, dw = 1;
    const int16_t* w[kMaxRes];     // [F][C*kh*kw] weights mod p_j
    const int8_t* w8[kMaxRes];     // [F][Kpad] centered int8 (MFMA path) or null
    int Kpad;
    const int32_t* zc[kMaxRes];    // [F]
    const int16_t* bias[kMaxRes];  // [B][F][n_j]
    const int16_t* zero;           // [B][lab_stride]
    int lab_stride;
    int lab_off[kMaxRes];
    int use_mfma;
    // LDS-image MFMA path (k_conv_img): weights [F16][kh][kw][Cpad] centered int8
    const int8_t* w8r[kMaxRes];
    int Cpad = 0, band = 0, nbands = 0;
    int64_t img_off[kMaxRes + 1];  // first image index of residue j: B * sum_{i<j} n_i
    uint32_t mq[kMaxRes];          // floor(2^32 / p_j): reciprocal for the epilogue's mod p (conv_img_geometry)
    // 24-bit reduction (conv_img_geometry): x mod p = x - p * mulhi_u24(x << sh24, m24) exactly when the
    // accumulator bound keeps x << sh24 below 2^24; sh24 = -1: the 32-bit reduction
    uint32_t m24[kMaxRes];
    int sh24[kMaxRes];
    int ldsS = 0, ldsR = 0;        // LDS image: bytes per position and per input row (conv_img_geometry)
    // tap-unrolled image (conv_unroll_taps): the band is staged per OUTPUT position with the C*kh*kw patch
    // bytes as its channels, the MFMA phase then runs a 1x1 conv (one k-step instead of kh*kw for C << 64).
    // u* hold the layer's own geometry for the staging; the fields above describe the unrolled view.
    int ur = 0;
    int uC = 0, uH = 0, uW = 0, ukh = 0, ukw = 0, ush = 0, usw = 0, uph = 0, upw = 0, udh = 1, udw = 1;
    // grouped conv (k_conv_grp, groups > 1; 0 and 1 are the dense paths above): group q holds filters
    // [q F/g, (q+1) F/g) and reads channels [q C/g, (q+1) C/g). wg: weights mod p_j as unsigned bytes (not
    // centered), [F][C/g][kh][ceil(kw/4)] dwords of 4 dx taps each, zero filled (dilated: [F][C/g][kh][kw] dwords
    // of one tap each in byte 0, conv_grp_kwd). Block geometry from
    // conv_grp_geometry: gpb groups and gband output rows per block, gR bytes per LDS image row, gnpp padded
    // lane slots per filter.
    int groups = 0;
    const uint32_t* wg[kMaxRes];
    int gpb = 0, gngb = 0, gband = 0, gnbands = 0, gR = 0, gnpp = 0;
    // transposed conv (layers.h ConvTGeom): the fields above describe its stride-1 sub-pixel view with
    // F = tF * tsh * tsw filters, and the epilogue scatters view output (f', qy, qx), f' = (f * tsh + ry) * tsw + rx,
    // to (f, tsh * qy + ry - tph, tsw * qx + rx - tpw) of the tF x tOH x tOW output; what falls outside is
    // dropped (depth-to-space + crop). tsc = 0: off (a plain conv); 1: byte stores; 2: tsw = 2 and lanes l, l ^ 1
    // exchange two bytes so each stores four adjacent output bytes (a dword where aligned), k_conv_img2 only.
    int tsc = 0, tsh = 1, tsw = 1, tph = 0, tpw = 0, tF = 0, tOH = 0, tOW = 0;
};
// Describe a transposed conv's view and scatter in `a` (shape fields only; plan it with conv_layer_plan next).
// wide: the exchanged four-byte store where it applies (tsw = 2; A/B knob DASH_CONVT_WIDE, default on)
inline bool convt_wide_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("DASH_CONVT_WIDE");
        return !(e && e[0] == '0');
    }();
    return on;
}
inline void convt_view_args(ConvArgs& a, int C, int H, int W, int F, int kh, int kw, int sh, int sw, int ph, int pw,
                            int OH, int OW) {
    const int Th = (kh + sh - 1) / sh, Tw = (kw + sw - 1) / sw;
    a.C = C; a.H = H; a.W = W;
    a.F = F * sh * sw;
    a.kh = Th; a.kw = Tw;
    a.sh = a.sw = 1;
    a.dh = a.dw = 1;
    a.ph = Th - 1; a.pw = Tw - 1;
    a.OH = H + Th - 1; a.OW = W + Tw - 1;
    a.groups = 0;
    a.tsc = (sw == 2 && convt_wide_enabled()) ? 2 : 1;
    a.tsh = sh; a.tsw = sw; a.tph = ph; a.tpw = pw;
    a.tF = F; a.tOH = OH; a.tOW = OW;
}
void launch_conv(const ConvArgs& a, const Act& x, const Act& y, int B, hipStream_t st);

// Input rows a band of `rows` output rows reads: from the first row's first tap to the last row's last tap. The ONE
// definition of the staged band height: the band-fits-budget loops (conv_img_geometry, conv_grp_lds), the dynamic
// LDS size (launch_conv) and the kernels' staging and tap loops all call it, so the image a kernel addresses is
// the image that was allocated.
__host__ __device__ inline int conv_band_in_rows(int rows, int sh, int kh, int dh) {
    return (rows - 1) * sh + (kh - 1) * dh + 1;
}
// Whether the layer runs a dilated kernel form (the tap-unrolled view carries the layer's own dilation in u*)
inline bool conv_dilated(const ConvArgs& a) { return a.ur ? (a.udh > 1 || a.udw > 1) : (a.dh > 1 || a.dw > 1); }

// k_conv_img geometry: 64-channel chunks (Cpad), the LDS image's position
// stride S and row stride R, and the tallest band of output rows whose input
// rows fit 64 KiB; nbands = 0 if none fits (launch_conv then uses the im2col
// MFMA kernel). S and R are chosen per layer by simulating the MFMA
// B-operand ds_read_b128 of the first 64 output columns over all taps under
// gfx950's banking (64 dword banks, 4 lane groups of 16:
// {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same +32): 4 LDS cycles per
// read is conflict-free. The image is stored channel-last with the staging
// lanes walking channels fastest (ds_write_b32 conflict-free for any S, R).
inline int conv_lds_read_cycles(const ConvArgs& a, int S, int R) {
    static const int G[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                 {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                 {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                 {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    int total = 0;
    for (int t = 0; t < 4; ++t)
        for (int dy = 0; dy < a.kh; ++dy)
            for (int dx = 0; dx < a.kw; ++dx)
                for (int g = 0; g < 4; ++g) {
                    // distinct dwords per bank: at most 16 lanes x 4 dwords land in 64 banks
                    int vals[64][16];
                    int cnt[64] = {0};
                    int worst = 1;
                    for (int i = 0; i < 16; ++i) {
                        const int l = G[g][i];
                        const int col = t * 16 + (l & 15), oy = col / a.OW, ox = col % a.OW;
                        const int base = ((oy * a.sh + dy * a.dh) * R + (ox * a.sw + dx * a.dw) * S + (l >> 4) * 16) / 4;
                        for (int d = 0; d < 4; ++d) {
                            const int dw = base + d, bk = dw & 63;
                            bool dup = false;
                            for (int q = 0; q < cnt[bk]; ++q) dup |= vals[bk][q] == dw;
                            if (!dup) {
                                vals[bk][cnt[bk]++] = dw;
                                worst = cnt[bk] > worst ? cnt[bk] : worst;
                            }
                        }
                    }
                    total += worst;
                }
    return total;
}

struct ConvGeomPick {
    int S, R, band, nbands;
};
inline void conv_img_geometry(ConvArgs& a) {
    a.Cpad = (a.C + 63) / 64 * 64;
    for (int j = 0; j < a.crt.k; ++j) {
        const int p = a.crt.p[j];
        a.mq[j] = static_cast<uint32_t>(0x100000000ull / static_cast<uint32_t>(p));
        // x = acc + epilogue constant < 2 * Kpad * half * xmax + (Kpad + 3) p (the epilogue's bound)
        const int half = p / 2;
        const uint64_t xmax = p < 128 ? static_cast<uint64_t>(p - 1) : static_cast<uint64_t>(half);
        const uint64_t X = 2ull * static_cast<uint64_t>(a.Kpad) * half * xmax + (static_cast<uint64_t>(a.Kpad) + 3) * p;
        // smallest sh with m = ceil(2^(32 - sh) / p) < 2^24, i.e. 2^(8 - sh) < p; then q = floor(x m / 2^(32 - sh))
        // is floor(x / p) exactly for x < 2^(24 - sh) and p < 256 (the rounding error stays below 2^-8 < 1 / p)
        a.sh24[j] = -1;
        a.m24[j] = 0;
        if (p >= 2 && p < 256) {
            int sh = 0;
            while (sh <= 8 && (1 << (8 - sh)) >= p) ++sh;
            if (sh <= 8 && X < (1ull << (24 - sh))) {
                const uint64_t m = ((1ull << (32 - sh)) + static_cast<uint64_t>(p) - 1) / static_cast<uint64_t>(p);
                if (m < (1ull << 24)) {
                    a.sh24[j] = sh;
                    a.m24[j] = static_cast<uint32_t>(m);
                }
            }
        }
    }
    // the pick depends on the layer shape only: computed once per shape and process (garbling calls this per GC)
    static std::mutex mu;
    static std::map<std::vector<int>, ConvGeomPick> memo;
    const std::vector<int> key{a.C, a.W, a.pw, a.OH, a.OW, a.kh, a.kw, a.sh, a.sw, a.dh, a.dw};
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = memo.find(key);
        if (it != memo.end()) {
            a.ldsS = it->second.S;
            a.ldsR = it->second.R;
            a.band = it->second.band;
            a.nbands = it->second.nbands;
            return;
        }
    }
    const int Wp = a.W + 2 * a.pw;
    // LDS budget per block (A/B knob DASH_CONV_LDS_KB, default 40: measured 64 KiB 21.0, 40 KiB 16.3, 32 KiB 17.9 ms of conv per MiniONN step at 102 GCs): smaller bands leave room for more
    // resident blocks, so one block's staging overlaps another's MFMAs
    static const int64_t budget = [] {
        const char* e = std::getenv("DASH_CONV_LDS_KB");
        const int64_t kb = e ? std::atoll(e) : 40;
        return std::max<int64_t>(8, std::min<int64_t>(64, kb)) * 1024;
    }();
    long best_cyc = -1, best_lds = 0;
    a.band = a.nbands = 0;
    for (int extra : {16, 32, 48, 80}) {
        const int S = a.Cpad + extra;
        for (int rpad = 0; rpad < 256; rpad += 16) {
            const int R = Wp * S + rpad;
            int band = a.OH;
            while (band > 1 && static_cast<int64_t>(conv_band_in_rows(band, a.sh, a.kh, a.dh)) * R > budget) --band;
            const int64_t lds = static_cast<int64_t>(conv_band_in_rows(band, a.sh, a.kh, a.dh)) * R;
            if (lds > budget) continue;
            const long cyc = conv_lds_read_cycles(a, S, R);
            if (best_cyc < 0 || cyc < best_cyc || (cyc == best_cyc && lds < best_lds)) {
                best_cyc = cyc;
                best_lds = lds;
                a.ldsS = S;
                a.ldsR = R;
                a.band = band;
                a.nbands = (a.OH + band - 1) / band;
            }
        }
    }
    std::lock_guard<std::mutex> lk(mu);
    memo[key] = ConvGeomPick{a.ldsS, a.ldsR, a.band, a.nbands};
}

// Switch a layer to the tap-unrolled image when that cuts the MFMA k-steps (few input channels, e.g. the
// RGB first layer: 3x3x3 = 27 patch bytes in one 64-wide k-step instead of 9 steps of 3 real channels each)
// and every residue takes the int8 MFMA path. Unit column stride only (the staging's 8-column loads; a dilated
// tap only shifts where the 8 columns start).
// Call before conv_img_geometry; the caller lays out w8r with conv_w8r.
inline void conv_unroll_taps(ConvArgs& a, int max_p) {
    const int K = a.C * a.kh * a.kw;
    const int steps = a.kh * a.kw * ((a.C + 63) / 64), usteps = (K + 63) / 64;
    const bool ok = [] {
        const char* e = std::getenv("DASH_CONV_UNROLL");
        return !(e && e[0] == '0');
    }();
    if (!ok || a.ur || a.sw != 1 || max_p > 255 || usteps >= steps || a.uW != 0) return;
    a.ur = 1;
    a.uC = a.C; a.uH = a.H; a.uW = a.W; a.ukh = a.kh; a.ukw = a.kw;
    a.ush = a.sh; a.usw = a.sw; a.uph = a.ph; a.upw = a.pw; a.udh = a.dh; a.udw = a.dw;
    a.C = K; a.H = a.OH; a.W = a.OW;
    a.kh = a.kw = a.sh = a.sw = a.dh = a.dw = 1;
    a.ph = a.pw = 0;
}

// Conv kernel geometry for a layer: the tap-unrolled view where it pays (conv_unroll_taps), the LDS band
// image otherwise; when no band of the unrolled view fits the LDS budget (wide outputs, small
// DASH_CONV_LDS_KB) the layer falls back to its own geometry (plain band image, or im2col when nbands = 0).
inline void conv_plan(ConvArgs& a, int max_p, bool unroll) {
    const ConvArgs own = a;
    if (unroll) conv_unroll_taps(a, max_p);
    conv_img_geometry(a);
    if (a.ur && a.nbands == 0) {
        a = own;
        conv_img_geometry(a);
    }
}

// The whole plan of a dense (groups <= 1) conv layer from its shape (C .. OW) and CRT base (a.crt): the padded
// reduction length, then conv_plan with the base's largest modulus. img: the LDS-image kernels may run (the
// evaluator's mfma switch and the DASH_CONV_IMG A/B knob; the GPU garbler always allows them); without them the
// layer takes the im2col MFMA or the VALU kernel (nbands = 0). The evaluator, the GPU garbler and the test
// binding hip_conv_plan all plan through this one function; it needs no device.
inline bool conv_img_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("DASH_CONV_IMG");
        return !(e && e[0] == '0');
    }();
    return on;
}
inline void conv_layer_plan(ConvArgs& a, bool img) {
    a.Kpad = (a.C * a.kh * a.kw + 63) / 64 * 64;
    int max_p = 0;
    for (int j = 0; j < a.crt.k; ++j) max_p = std::max(max_p, a.crt.p[j]);
    conv_plan(a, max_p, img);
    if (!img) a.band = a.nbands = 0;
}

// k_conv_grp geometry. A lane owns 4 adjacent output columns of one (filter, row); a block owns one image,
// gband output rows and gpb consecutive groups:
//   * band rule: the whole plane if its OH * ceil(OW/4) lane slots fit the block's 256 lanes, else the most
//     rows that do (at least one);
//   * gnpp: a filter's slots padded to a multiple of 64 (the filter is then wave-uniform: its weight reads
//     from LDS are broadcasts) or, below 64, to a power of two (several filters per wave);
//   * gpb: as many groups as fill the 256 lanes kGrpPasses times over (a lane loops over its slots: one
//     staging pass and one barrier then serve several outputs per lane; one pass per block left the layer
//     bound by block start-up), at most kGrpMaxGroups, shrunk until the staged rows and weights fit 16 KiB of LDS
//     (several blocks per CU);
//   * the band then shrinks until a single group's rows and weights fit 64 KiB.
// gR covers the padded row and the furthest dword any lane reads, in 16-byte staging chunks.
// Dilated layers (dh > 1 or dw > 1) hold one tap per weight dword (conv_grp_kwd = kw): the four adjacent dx taps
// of a dot4 are not adjacent bytes there. A lane's furthest tap is then (kw - 1) dw bytes past its last window.
// Returns the dynamic LDS bytes (rows, weights, constants), or 0 when even one group and one output row do not fit.
constexpr int kGrpPasses = 8, kGrpMaxGroups = 32;
// weight dwords per kernel row: 4 dx taps per dword, or one per dword when dilated
inline int conv_grp_kwd(int kw, bool dilated) { return dilated ? kw : (kw + 3) / 4; }
inline size_t conv_grp_lds(const ConvArgs& a, int gpb, int band) {
    const int Cg = a.C / a.groups, Fg = a.F / a.groups;
    const size_t img = static_cast<size_t>(gpb) * Cg * conv_band_in_rows(band, a.sh, a.kh, a.dh) * a.gR;
    // the groups' weight dwords and one epilogue constant per filter
    const size_t wl =
        static_cast<size_t>(gpb) * Fg * (static_cast<size_t>(Cg) * a.kh * conv_grp_kwd(a.kw, conv_dilated(a)) + 1) * 4;
    return img + wl;
}
inline int conv_grp_npp(const ConvArgs& a, int band) {
    const int np = band * ((a.OW + 3) / 4);
    if (np >= 64) return (np + 63) / 64 * 64;
    int v = 1;
    while (v < np) v *= 2;
    return v;
}
inline size_t conv_grp_geometry(ConvArgs& a) {
    for (int j = 0; j < a.crt.k; ++j)
        a.mq[j] = static_cast<uint32_t>(0x100000000ull / static_cast<uint32_t>(a.crt.p[j]));
    const int OWq = (a.OW + 3) / 4, kwd = (a.kw + 3) / 4, Fg = a.F / a.groups;
    // the last lane's last window starts at byte 4 (OWq - 1) sw + 3 sw; packed taps read the dwords covering
    // 4 kwd more bytes, a dilated tap the dword that holds byte (kw - 1) dw past it
    const int ext = conv_dilated(a) ? 4 * (OWq - 1) * a.sw + 3 * a.sw + (a.kw - 1) * a.dw + 4
                                    : 4 * (OWq - 1) * a.sw + 3 * a.sw + 4 * kwd + 4;
    a.gR = (std::max(a.W + 2 * a.pw, ext) + 15) / 16 * 16;
    const size_t budget = 64 * 1024;
    int band = a.OH;
    if (static_cast<int64_t>(a.OH) * OWq > 256) band = std::max(1, 256 / OWq);
    int64_t lanes = static_cast<int64_t>(Fg) * conv_grp_npp(a, band);
    int gpb = static_cast<int>(std::max<int64_t>(
        1, std::min<int64_t>(std::min(a.groups, kGrpMaxGroups), (256 * kGrpPasses + lanes - 1) / lanes)));
    while (gpb > 1 && conv_grp_lds(a, gpb, band) > 16 * 1024) --gpb;
    while (band > 1 && conv_grp_lds(a, gpb, band) > budget) --band;
    a.gpb = gpb;
    a.gngb = (a.groups + gpb - 1) / gpb;
    a.gband = band;
    a.gnbands = (a.OH + band - 1) / band;
    a.gnpp = conv_grp_npp(a, band);
    const size_t lds = conv_grp_lds(a, gpb, band);
    return lds > budget ? 0 : lds;
}
// k_conv_grp weight image of residue p from the [F][C/g][kh][kw] weights (reduced, non-negative); dilated: one
// tap per dword, in byte 0
inline std::vector<uint32_t> conv_grp_weights(const int64_t* w, int64_t F, int64_t Cg, int kh, int kw, int p,
                                              bool dilated = false) {
    const int kwd = conv_grp_kwd(kw, dilated);
    std::vector<uint32_t> r(static_cast<size_t>(F * Cg) * kh * kwd, 0u);
    for (int64_t fc = 0; fc < F * Cg; ++fc)
        for (int dy = 0; dy < kh; ++dy)
            for (int dx = 0; dx < kw; ++dx) {
                const uint32_t v = static_cast<uint32_t>(w[(fc * kh + dy) * kw + dx] % p);
                if (dilated) r[(static_cast<size_t>(fc) * kh + dy) * kwd + dx] = v;
                else r[(static_cast<size_t>(fc) * kh + dy) * kwd + dx / 4] |= v << (8 * (dx % 4));
            }
    return r;
}

// MFMA weight image [F16][kh][kw][Cpad] from the centered im2col weights w8 [F][Kpad] (order ci*kh*kw + dy*kw
// + dx); tap-unrolled layers: [F16][Cpad] with patch channel (dy*kw + dx)*C + ci (the staging's order)
inline std::vector<int8_t> conv_w8r(const ConvArgs& a, const std::vector<int8_t>& w8, int F) {
    const int F16 = (F + 15) / 16 * 16;
    const int C = a.ur ? a.uC : a.C, kh = a.ur ? a.ukh : a.kh, kw = a.ur ? a.ukw : a.kw;
    std::vector<int8_t> r(static_cast<size_t>(F16) * a.kh * a.kw * a.Cpad, 0);
    for (int f = 0; f < F; ++f)
        for (int ci = 0; ci < C; ++ci)
            for (int dy = 0; dy < kh; ++dy)
                for (int dx = 0; dx < kw; ++dx) {
                    const size_t dst = a.ur ? static_cast<size_t>(f) * a.Cpad + (dy * kw + dx) * C + ci
                                            : ((static_cast<size_t>(f) * kh + dy) * kw + dx) * a.Cpad + ci;
                    r[dst] = w8[static_cast<size_t>(f) * a.Kpad + (ci * kh + dy) * kw + dx];
                }
    return r;
}

// int16 matrix transpose out[c][r] = in[r][c] (label-major <-> component-major), kernels_label.hip
void launch_transpose16(const int16_t* in, int16_t* out, int64_t rows, int64_t cols, hipStream_t st);
void launch_narrow(const int16_t* in, act_t* out, int64_t n, hipStream_t st);  // int16 labels -> byte activations
void launch_encode_in(const EncIn& a, const int64_t* x, int64_t N, int slots, hipStream_t st);  // garbler: W0 + x R
void launch_transpose_to_act(const int16_t* in, act_t* out, int64_t rows, int64_t cols, hipStream_t st);
void launch_transpose_from_act(const act_t* in, int16_t* out, int64_t rows, int64_t cols, hipStream_t st);
// the same for every residue of a label set in one launch (grid z = residue): matrix j is rows[j] x cols[j]
struct TrRes {
    const void* in[kMaxRes];
    void* out[kMaxRes];
    int64_t rows[kMaxRes], cols[kMaxRes];
    int k;
};
void launch_transpose_to_act_res(const TrRes& a, hipStream_t st);    // int16 -> bytes
void launch_transpose_from_act_res(const TrRes& a, hipStream_t st);  // bytes -> int16
// elementwise casts of rows[j] * cols[j] contiguous components per residue (layouts already match)
void launch_cast_to_act_res(const TrRes& a, hipStream_t st);    // int16 -> bytes
void launch_cast_from_act_res(const TrRes& a, hipStream_t st);  // bytes -> int16
// per-slot constant scatter (HipEvaluator::load): block i copies `bytes` from src + off to dst0 + b * stride
struct ScatterDesc {
    size_t off;
    uint8_t* dst0;
    size_t stride, bytes;
};
void launch_scatter(const ScatterDesc* d, int n, const uint8_t* src, int b, hipStream_t st);
// the GPU garbler's chunked labels (component q of element e at ((q / 8) * N + e) * 8 + q % 8; rows[j] = n_j,
// cols[j] = N) <-> component-major bytes [n][N]
void launch_unchunk_to_act_res(const TrRes& a, hipStream_t st);
void launch_chunk_from_act_res(const TrRes& a, hipStream_t st);

}  // namespace dev
}  // namespace dash
