// Layer geometry shared by garbler, host evaluator and HIP runtime.
#pragma once

#include "model.h"

namespace dash {

struct ConvGeom {
    // g channel groups: group q holds filters [q*F/g, (q+1)*F/g) and reads
    // channels [q*C/g, (q+1)*C/g); weights are [F][C/g][kh][kw]
    i64 C, H, W, F, kh, kw, sh, sw, ph, pw, OH, OW, g;
    explicit ConvGeom(const Params& p);
    explicit ConvGeom(const GLayer& g) : ConvGeom(g.p) {}
    i64 Cg() const { return C / g; }
    i64 Fg() const { return F / g; }
    i64 K() const { return (C / g) * kh * kw; }
    i64 out_size() const { return F * OH * OW; }
};

struct PoolGeom {
    // ph/pw: symmetric padding (at most half the kernel); ceil: ONNX/PyTorch ceil_mode output size
    i64 C, H, W, kh, kw, sh, sw, ph, pw, ceil, OH, OW;
    explicit PoolGeom(const Params& p);
    i64 out_size() const { return C * OH * OW; }
    bool padded() const { return ph || pw || ceil; }
    // flattened input indices of output element o's window (row-major), always kh*kw of them: a tap outside
    // the image is replaced by the tap at the clamped coordinate, which lies in the same window (max pooling)
    void window(i64 o, std::vector<i64>& idx) const;
    // the in-image taps only (sum pooling); at least one, at most kh*kw
    void window_inside(i64 o, std::vector<i64>& idx) const;
};

// Pairwise max-reduction schedule over a window of K values: level l has
// ops[l] pair-max operations; value slots after level l: cnt[l+1].
struct MaxTree {
    std::vector<int> ops, cnt;
    explicit MaxTree(i64 K);
};

inline i64 param1(const Params& p, const char* k, i64 dflt = -1) {
    auto it = p.find(k);
    return (it == p.end() || it->second.empty()) ? dflt : it->second[0];
}
inline const std::vector<i64>& paramv(const Params& p, const char* k) {
    auto it = p.find(k);
    DASH_CHECK(it != p.end(), std::string("missing param ") + k);
    return it->second;
}

// dense input remap for TF (NHWC) flattening: reference cuda_util.h:130
inline i64 dense_src(i64 i, i64 K, i64 ch) { return ch > 0 ? i / ch + (i % ch) * (K / ch) : i; }

std::string arr_name(const char* prefix, int idx, const char* suffix);

}  // namespace dash
