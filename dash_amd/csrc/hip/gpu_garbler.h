// GPU garbler (see garble_gpu.hip). Plain C++ interface so the host garbler
// (garbler.cpp) can dispatch to it.
//
// The garbler's current base labels live on the device between GPU layers
// ("device cur"): the host garbler calls to_device() before a GPU layer when
// its host copy is newer and to_host() before a host layer when the device
// copy is newer, so a run of GPU layers (conv -> rescale -> ReLU -> conv ...)
// never moves labels over PCIe. GPU layers leave the host `cur` stale: they
// only set its shape (p, n, N) and clear its storage.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "../gadgets.h"
#include "../layers.h"

namespace dash {

class GpuGarbler {
   public:
    // hardened: the tables use the hardened encoding's tweaked pads (core.h hard_block) instead of H(K)
    GpuGarbler(const std::vector<int>& crt, const std::vector<int>& mrs, const std::string& seed16, const LabelBank& R,
               const LabelBank& Z, int device, bool hardened = false);
    ~GpuGarbler();
    void to_device(const CrtLabels& cur);
    void to_host(CrtLabels& cur);
    // conv base labels: y = sum_{w != 0 mod p} w*x + (1 + #zero weights)*Z_p (padding reads Z_p);
    // w are the weights reduced mod M ([F][C][kh][kw]), wh their hash_i64 (plan cache key)
    void conv(const ConvGeom& G, const i64* w, size_t nw, uint64_t wh, CrtLabels& cur);
    // ReLU (relu_crt/prefix/mmg/mme set) or Sign layer: tables; device cur -> next base labels
    void sign_layer(uint64_t layer, const SignPlan& sp, CrtLabels& cur, Array& ap, Array& c1, Array& c2, Array& sg,
                    const std::vector<int>* relu_crt, const std::vector<i64>* prefix, Array* mmg, Array* mme);
    // one DASH legacy rescale iteration (sign base extension) on the device cur, in place
    void rescale_legacy_iter(uint64_t layer, int it, const RescalePlan& P, CrtLabels& cur,
                             const std::vector<std::vector<comp_t>>& up, const std::vector<std::vector<comp_t>>& down,
                             Array& tr, Array& ap, Array& c1, Array& c2, Array& sg);

    // legacy rescale as one mixed-radix gadget (gadgets.h RescaleMrsPlan) on the device cur, in place
    void rescale_mrs(uint64_t layer, const RescaleMrsPlan& P, CrtLabels& cur, Array& tab);

    // ReLU with the exact mixed-radix sign (gadgets.h SignMrsPlan) + mixed-modulus half gates; device cur -> next
    void relu_mrs(uint64_t layer, const SignMrsPlan& P, CrtLabels& cur, Array& tab, const std::vector<int>* relu_crt,
                  const std::vector<i64>* prefix, Array& mmg, Array& mme);

    // Clip (gadgets.h ClipPlan): two signs, exact (pm; tables st[side][0] = mrs) or approximate (pa; st[side] =
    // approx, cast2, sign), side 0 = lower bound; the half gates keyed by u = s_lo + s_hi and the cap rows keyed by
    // s_hi; device cur -> next. Registered by the device translation unit like concat_saved, so host-only links
    // need no definition.
    using ClipFn = void (*)(GpuGarbler&, uint64_t, const SignMrsPlan*, const SignPlan*, i64, i64, CrtLabels&,
                            Array* const (*)[3], const std::vector<i64>*, Array&, Array&, Array&);
    static ClipFn& clip_hook() {
        static ClipFn f = nullptr;
        return f;
    }
    void clip(uint64_t layer, const SignMrsPlan* pm, const SignPlan* pa, i64 lo, i64 hi, CrtLabels& cur,
              Array* const (*st)[3], const std::vector<i64>* prefix, Array& mmg, Array& mme, Array& cap) {
        DASH_CHECK(clip_hook() != nullptr, "gpu garbler: clip is not linked in");
        clip_hook()(*this, layer, pm, pa, lo, hi, cur, st, prefix, mmg, mme, cap);
    }

    // Joint Clip (gadgets.h ClipPlan, joint variant), two calls around the rescale_mrs of the layer before it.
    // clip_hi_sign, before that rescale: the exact sign of x - t_hi on the device cur (the rescale's input; the
    // shift folded in and out again), PRG stream and gate of the Clip layer's slot 3, tables -> tab; its mod-2
    // base labels are kept on the device, and the rescale_mrs that follows keeps a copy of its own sign label
    // beside them. clip_joint, at the Clip: u = the two kept labels' sum, the half gates, the cap rows keyed by
    // the kept upper sign, and the output base labels; device cur -> next. Hooks as for clip.
    using ClipHiFn = void (*)(GpuGarbler&, uint64_t, const SignMrsPlan&, i64, CrtLabels&, Array&);
    using ClipJointFn = void (*)(GpuGarbler&, uint64_t, i64, CrtLabels&, const std::vector<i64>*, Array&, Array&,
                                 Array&);
    static ClipHiFn& clip_hi_hook() {
        static ClipHiFn f = nullptr;
        return f;
    }
    static ClipJointFn& clip_joint_hook() {
        static ClipJointFn f = nullptr;
        return f;
    }
    void clip_hi_sign(uint64_t layer, const SignMrsPlan& pm, i64 t_hi, CrtLabels& cur, Array& tab) {
        DASH_CHECK(clip_hi_hook() != nullptr, "gpu garbler: clip is not linked in");
        clip_hi_hook()(*this, layer, pm, t_hi, cur, tab);
    }
    void clip_joint(uint64_t layer, i64 hi, CrtLabels& cur, const std::vector<i64>* prefix, Array& mmg, Array& mme,
                    Array& cap) {
        DASH_CHECK(clip_joint_hook() != nullptr, "gpu garbler: clip is not linked in");
        clip_joint_hook()(*this, layer, hi, cur, prefix, mmg, mme, cap);
    }

    // ReLU whose sign labels the preceding rescale_mrs (P.sign_last) left on the device: mixed-modulus half
    // gates only; device cur -> next
    void relu_mult(uint64_t layer, CrtLabels& cur, const std::vector<i64>* prefix, Array& mmg, Array& mme);

    // dense base labels y_o = sum_{w != 0 mod p} w x_src(i) + (1 + #zero weights) Z_p (w reduced mod M, [out][in],
    // src = dense_src(i, in, channel_tf))
    void dense(i64 in, i64 out, i64 channel_tf, const i64* w, size_t nw, uint64_t wh, CrtLabels& cur);
    // hardened encoding: cur_e += (c[e / group] mod p) R_p (public constants folded into the base labels)
    void fold_constants(const std::vector<i64>& c, i64 group, CrtLabels& cur);
    // window sums of the device cur
    void sumpool(const PoolGeom& G, CrtLabels& cur);
    // device copies of layer outputs a later residual add / in_src layer reads (idx = layer index + 1)
    void save(size_t idx);
    bool has_saved(size_t idx) const;
    void restore(size_t idx, CrtLabels& cur);
    void add_saved(size_t idx, CrtLabels& cur);
    // cur = the saved outputs idx[0], idx[1], ... concatenated (channel concat of [C][H][W] tensors). The device
    // translation unit registers the implementation, so host-only links of garbler.cpp (which never construct a
    // GpuGarbler) need no definition of it.
    using ConcatFn = void (*)(GpuGarbler&, const std::vector<size_t>&, CrtLabels&);
    static ConcatFn& concat_hook() {
        static ConcatFn f = nullptr;
        return f;
    }
    void concat_saved(const std::vector<size_t>& idx, CrtLabels& cur) {
        DASH_CHECK(concat_hook() != nullptr, "gpu garbler: concat is not linked in");
        concat_hook()(*this, idx, cur);
    }
    // Transposed conv base labels (hardened encoding: the bare sum over the valid taps; the caller folds the bias):
    // the evaluator's launch_conv on the layer's sub-pixel view (layers.h ConvTGeom), w [C][F][kh][kw] reduced
    // mod M, wh their hash. Upsample: a gather of the device cur. Hooks as for concat_saved.
    using ConvTFn = void (*)(GpuGarbler&, const ConvTGeom&, const i64*, size_t, uint64_t, CrtLabels&);
    using UpsampleFn = void (*)(GpuGarbler&, const UpGeom&, CrtLabels&);
    static ConvTFn& convt_hook() {
        static ConvTFn f = nullptr;
        return f;
    }
    static UpsampleFn& upsample_hook() {
        static UpsampleFn f = nullptr;
        return f;
    }
    void conv_transpose(const ConvTGeom& G, const i64* w, size_t nw, uint64_t wh, CrtLabels& cur) {
        DASH_CHECK(convt_hook() != nullptr, "gpu garbler: conv_transpose2d is not linked in");
        convt_hook()(*this, G, w, nw, wh, cur);
    }
    void upsample(const UpGeom& G, CrtLabels& cur) {
        DASH_CHECK(upsample_hook() != nullptr, "gpu garbler: upsample is not linked in");
        upsample_hook()(*this, G, cur);
    }
    // Gather (K_GATHER): cur[o] = the device cur[idx[o]], on whatever moduli cur carries. A hook as for upsample.
    using GatherFn = void (*)(GpuGarbler&, const std::vector<i64>&, CrtLabels&);
    static GatherFn& gather_hook() {
        static GatherFn f = nullptr;
        return f;
    }
    void gather(const std::vector<i64>& idx, CrtLabels& cur) {
        DASH_CHECK(gather_hook() != nullptr, "gpu garbler: gather is not linked in");
        gather_hook()(*this, idx, cur);
    }
    // Bilinear (K_BILINEAR): cur = the layer's public two-tap stencil on the device cur, through the evaluator's own
    // kernels (launch_bilinear). A hook as for upsample.
    using BilinearFn = void (*)(GpuGarbler&, const BilinearGeom&, CrtLabels&);
    static BilinearFn& bilinear_hook() {
        static BilinearFn f = nullptr;
        return f;
    }
    void bilinear(const BilinearGeom& G, CrtLabels& cur) {
        DASH_CHECK(bilinear_hook() != nullptr, "gpu garbler: bilinear is not linked in");
        bilinear_hook()(*this, G, cur);
    }
    // max pool / max: window values, one ReLU-gadget tree level per call (relu_garble_elem on streams
    // 20 + 2 lv / 21 + 2 lv), then the reduced values become cur
    void maxpool_begin(const std::vector<std::vector<i64>>& win, CrtLabels& cur);
    void maxpool_level(uint64_t layer, int lv, i64 ops, const SignPlan& sp, const std::vector<i64>& prefix, Array& ap,
                       Array& c1, Array& c2, Array& sg, Array& mmg, Array& mme);
    void maxpool_end(CrtLabels& cur);
    // ArgMax (gadgets.h ArgMaxPlan), one tournament level over P positions: level 0 takes the device cur as the
    // candidates' values, the root leaves the index labels as the device cur. Tables of the level: mrs; mmg, mme
    // (empty at the root); idx (level 0) or img, ime (later levels). A hook as for clip, so host-only links need
    // no definition.
    using ArgMaxFn = void (*)(GpuGarbler&, uint64_t, int, const ArgMaxPlan&, i64, const std::vector<i64>&, CrtLabels&,
                              Array&, Array&, Array&, Array&, Array&, Array&);
    static ArgMaxFn& argmax_hook() {
        static ArgMaxFn f = nullptr;
        return f;
    }
    void argmax_level(uint64_t layer, int lv, const ArgMaxPlan& ap, i64 P, const std::vector<i64>& prefix,
                      CrtLabels& cur, Array& mrs, Array& mmg, Array& mme, Array& idx, Array& img, Array& ime) {
        DASH_CHECK(argmax_hook() != nullptr, "gpu garbler: argmax is not linked in");
        argmax_hook()(*this, layer, lv, ap, P, prefix, cur, mrs, mmg, mme, idx, img, ime);
    }
    // Mul (gadgets.h MulPlan): x = the device cur, y = the saved output `src_idx` (unused for a square); tables g, e
    // (product) or g = t (square); device cur -> next. A hook as for clip.
    using MulFn = void (*)(GpuGarbler&, uint64_t, const MulPlan&, size_t, CrtLabels&, Array&, Array&);
    static MulFn& mul_hook() {
        static MulFn f = nullptr;
        return f;
    }
    // x and y enter the projection descriptors as input residues j and k + j of one 16-entry set: a product needs
    // 2 k <= 16, a square k <= 16. The host garbler takes the layers that do not fit.
    static bool mul_fits(int k, bool square) { return (square ? k : 2 * k) <= 16; }
    // Mixed-radix rescale (gadgets.h RescaleMrsPlan): the emit kernel stages one element's last table row, T = 2^(l+1)
    // colors by k targets, in LDS with its position map, bank indices, pad runs and two elements' key hashes. An upper
    // estimate of that scope against the 64 KiB less the projection descriptors: k = 7 fits up to l = 8. A rescale
    // beyond it (a Rescale(l + e) that absorbs pending scale bits) garbles on the host, byte-identical.
    static bool rescale_mrs_fits(const std::vector<int>& crt, i64 l) {
        if (l < 0 || l > 11) return false;
        const i64 T = i64(2) << l, k = static_cast<i64>(crt.size());
        i64 nb = 0;
        for (int p : crt) nb += std::min<i64>(T, p);
        const i64 per = T * 20 + nb * 16;
        const i64 fixed = T * k * 6 + 16 + T * ((k + 3) / 4 + 1) * 4 + 4;
        return 2 * per + fixed <= (i64(64) << 10) - 32 * 224;
    }
    void mul(uint64_t layer, const MulPlan& mp, size_t src_idx, CrtLabels& cur, Array& g, Array& e) {
        DASH_CHECK(mul_hook() != nullptr, "gpu garbler: mul is not linked in");
        mul_hook()(*this, layer, mp, src_idx, cur, g, e);
    }
    // MatMul (gadgets.h MatMulPlan): x = the device cur (M T elements), y = the saved output `src_idx` (T N); tables
    // g, e [M N T][P]; device cur -> the M N outputs. Both operands are gathered to one zero label per product, the
    // products are Mul's (stream element o T + t) and each output's T product labels are summed. A hook as for mul.
    using MatMulFn = void (*)(GpuGarbler&, uint64_t, const MatMulPlan&, size_t, CrtLabels&, Array&, Array&);
    static MatMulFn& matmul_hook() {
        static MatMulFn f = nullptr;
        return f;
    }
    // The gathered operands and the products' slots live in device memory all at once: layers of more products
    // than this (and bases beyond mul_fits) garble on the host
    static constexpr i64 kMatMulMaxProducts = i64(1) << 18;  // about 5 KiB of labels and slots per product at k = 7
    static bool matmul_fits(int k, i64 products) { return mul_fits(k, false) && products <= kMatMulMaxProducts; }
    void matmul(uint64_t layer, const MatMulPlan& mp, size_t src_idx, CrtLabels& cur, Array& g, Array& e) {
        DASH_CHECK(matmul_hook() != nullptr, "gpu garbler: matmul is not linked in");
        matmul_hook()(*this, layer, mp, src_idx, cur, g, e);
    }
    // PiecewiseLinear (gadgets.h PwlPlan): per kept breakpoint i the device cur shifted to x0 + T_i R, the sign's
    // draw / derive / fan-out passes on stream slot 1 + 2i (pm: exact, pa: approximate fused) and the ReLU half
    // gates on slot 2 + 2i, each breakpoint's output zero labels added into the combination
    // a0 x0 + sum_i d_i t_i - c R, which becomes the device cur. t: five arrays per breakpoint (mrs | approx,
    // cast2, sign; mm.g; mm.e). Hook as for clip.
    using PwlFn = void (*)(GpuGarbler&, uint64_t, const PwlPlan&, const SignMrsPlan*, const SignPlan*, CrtLabels&,
                           const std::vector<Array*>&, const std::vector<i64>*);
    static PwlFn& pwl_hook() {
        static PwlFn f = nullptr;
        return f;
    }
    void pwl(uint64_t layer, const PwlPlan& pp, const SignMrsPlan* pm, const SignPlan* pa, CrtLabels& cur,
             const std::vector<Array*>& t, const std::vector<i64>* prefix) {
        DASH_CHECK(pwl_hook() != nullptr, "gpu garbler: pwl is not linked in");
        pwl_hook()(*this, layer, pp, pm, pa, cur, t, prefix);
    }
    // LeakyRelu (gadgets.h LeakyPlan), two calls around the ReLU garbling of the same layer (sign_layer, relu_mrs
    // or relu_mult): leaky_keep copies the device cur (the input zero labels x0) aside, leaky_map turns the ReLU's
    // output zero labels into (n_c mod p) x0 + ((2^s - n_c) mod p) relu0 in place. Hooks as for clip.
    using LeakyKeepFn = void (*)(GpuGarbler&, CrtLabels&);
    using LeakyMapFn = void (*)(GpuGarbler&, const LeakyPlan&, CrtLabels&);
    static LeakyKeepFn& leaky_keep_hook() {
        static LeakyKeepFn f = nullptr;
        return f;
    }
    static LeakyMapFn& leaky_map_hook() {
        static LeakyMapFn f = nullptr;
        return f;
    }
    void leaky_keep(CrtLabels& cur) {
        DASH_CHECK(leaky_keep_hook() != nullptr, "gpu garbler: leaky_relu is not linked in");
        leaky_keep_hook()(*this, cur);
    }
    void leaky_map(const LeakyPlan& lp, CrtLabels& cur) {
        DASH_CHECK(leaky_map_hook() != nullptr, "gpu garbler: leaky_relu is not linked in");
        leaky_map_hook()(*this, lp, cur);
    }
    // ReDash rescale iteration (base-extension plan) on the device cur, in place
    void rescale_redash(uint64_t layer, int it, const RescalePlan& P, CrtLabels& cur,
                        const std::vector<std::vector<comp_t>>& up, const std::vector<std::vector<comp_t>>& down,
                        Array& tr, Array& be);
    // base-extension layer on the device cur, in place
    void base_ext(uint64_t layer, const BEPlan& P, CrtLabels& cur, Array& be);

    struct Impl;

   private:
    // conv and conv_transpose: T set = G is T's sub-pixel view and w T's own weights
    void conv_run(const ConvGeom& G, const ConvTGeom* T, const i64* w, size_t nw, uint64_t wh, CrtLabels& cur);
    static void convt_dev(GpuGarbler& self, const ConvTGeom& G, const i64* w, size_t nw, uint64_t wh, CrtLabels& cur);
    static void upsample_dev(GpuGarbler& self, const UpGeom& G, CrtLabels& cur);
    static void gather_dev(GpuGarbler& self, const std::vector<i64>& idx, CrtLabels& cur);
    static void bilinear_dev(GpuGarbler& self, const BilinearGeom& G, CrtLabels& cur);
    static void concat_saved_dev(GpuGarbler& self, const std::vector<size_t>& idx, CrtLabels& cur);
    static void clip_dev(GpuGarbler& self, uint64_t layer, const SignMrsPlan* pm, const SignPlan* pa, i64 lo, i64 hi,
                         CrtLabels& cur, Array* const (*st)[3], const std::vector<i64>* prefix, Array& mmg, Array& mme,
                         Array& cap);
    static void clip_hi_dev(GpuGarbler& self, uint64_t layer, const SignMrsPlan& pm, i64 t_hi, CrtLabels& cur,
                            Array& tab);
    static void clip_joint_dev(GpuGarbler& self, uint64_t layer, i64 hi, CrtLabels& cur, const std::vector<i64>* prefix,
                               Array& mmg, Array& mme, Array& cap);
    static void argmax_level_dev(GpuGarbler& self, uint64_t layer, int lv, const ArgMaxPlan& ap, i64 P,
                                 const std::vector<i64>& prefix, CrtLabels& cur, Array& mrs, Array& mmg, Array& mme,
                                 Array& idx, Array& img, Array& ime);
    static void pwl_dev(GpuGarbler& self, uint64_t layer, const PwlPlan& pp, const SignMrsPlan* pm, const SignPlan* pa,
                        CrtLabels& cur, const std::vector<Array*>& t, const std::vector<i64>* prefix);
    static void leaky_keep_dev(GpuGarbler& self, CrtLabels& cur);
    static void leaky_map_dev(GpuGarbler& self, const LeakyPlan& lp, CrtLabels& cur);
    static void mul_dev(GpuGarbler& self, uint64_t layer, const MulPlan& mp, size_t src_idx, CrtLabels& cur, Array& g,
                        Array& e);
    static void matmul_dev(GpuGarbler& self, uint64_t layer, const MatMulPlan& mp, size_t src_idx, CrtLabels& cur,
                           Array& g, Array& e);
    std::unique_ptr<Impl> impl_;
};

// Device blocks of garbled tables freed by their owners return to a small
// per-process cache (exact-size reuse: every GC of one model has the same
// table sizes), so back-to-back garbling skips the driver's allocate-and-clear
// of fresh HBM. Bounded by DASH_GG_CACHE_GB (default 16); trim releases it.
void gpu_table_cache_trim();
size_t gpu_table_cache_bytes();

// The GPU garbler's launch record (garble_gpu.hip, host side only; off by default, one relaxed load per line
// that would be written). A list of its own beside the evaluator's launch log (launch.h): one line per gadget
// entry point, draw launch, capped launch and projection set (key path, scopes, compress_xa classes). take
// returns the lines recorded so far and clears them. gpu_garbler_compress_class: the record's name of the
// compress_xa form a modulus takes ("g8", "g4", "rt<digits per group>", "pw2"), from the
// predicate the kernels dispatch on; it needs no device.
void gpu_garbler_log_enable(bool on);
std::vector<std::string> gpu_garbler_log_take();
std::string gpu_garbler_compress_class(int q);

}  // namespace dash
