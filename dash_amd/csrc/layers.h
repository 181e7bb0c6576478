// Layer geometry shared by garbler, host evaluator and HIP runtime.
#pragma once

#include "model.h"

namespace dash {

struct ConvGeom {
    // g channel groups: group q holds filters [q*F/g, (q+1)*F/g) and reads
    // channels [q*C/g, (q+1)*C/g); weights are [F][C/g][kh][kw]. dh, dw: dilation (atrous conv), tap (dy, dx) of
    // output (oy, ox) reads input (oy sh - ph + dy dh, ox sw - pw + dx dw); a kernel axis of size 1 has dilation 1
    i64 C, H, W, F, kh, kw, sh, sw, ph, pw, OH, OW, g, dh, dw;
    explicit ConvGeom(const Params& p);
    explicit ConvGeom(const GLayer& g) : ConvGeom(g.p) {}
    i64 Cg() const { return C / g; }
    i64 Fg() const { return F / g; }
    i64 K() const { return (C / g) * kh * kw; }
    i64 out_size() const { return F * OH * OW; }
};

// Transposed convolution (PyTorch / ONNX ConvTranspose2d, groups = 1, no dilation): weights [C][F][kh][kw],
//   y[f][oy][ox] = b[f] + sum w[c][f][dy][dx] x[c][iy][ix] over the taps with oy + ph - dy = sh iy, 0 <= iy < H
// (likewise in x), OH = (H - 1) sh - 2 ph + kh + oph. Domain: 0 <= ph <= kh - 1, 0 <= oph < sh and
// oph <= sh Th - kh + ph with Th = ceil(kh / sh) (every output row is reached by the sub-pixel view below).
//
// Sub-pixel view (the HIP path): a stride-1 conv with VF = F sh sw filters f' = f sh sw + ry sw + rx, kernel
// Th x Tw, pads (Th - 1, Tw - 1), weights wv[f'][c][ty][tx] = w[c][f][ry + sh (Th-1-ty)][rx + sw (Tw-1-tx)] (zero
// past kh / kw); view output (f', qy, qx) is y[f][sh qy + ry - ph][sw qx + rx - pw] where that lies inside.
struct ConvTGeom {
    i64 C, H, W, F, kh, kw, sh, sw, ph, pw, oph, opw, OH, OW, Th, Tw;
    explicit ConvTGeom(const Params& p);
    explicit ConvTGeom(const GLayer& g) : ConvTGeom(g.p) {}
    i64 K() const { return C * kh * kw; }
    i64 out_size() const { return F * OH * OW; }
    i64 VF() const { return F * sh * sw; }
    i64 VK() const { return C * Th * Tw; }
    ConvGeom view() const;
    // [VF][C][Th][Tw] from w [C][F][kh][kw]
    std::vector<i64> view_weights(const i64* w) const;
};

// Nearest-neighbour upsampling by integer factors: y[c][oy][ox] = x[c][oy / fh][ox / fw]
struct UpGeom {
    i64 C, H, W, fh, fw;
    explicit UpGeom(const Params& p);
    i64 out_size() const { return C * H * fh * W * fw; }
    i64 src(i64 o) const {
        const i64 OW = W * fw, OH = H * fh;
        const i64 c = o / (OH * OW), r = o % (OH * OW);
        return (c * H + (r / OW) / fh) * W + (r % OW) / fw;
    }
};

// General gather of a flat tensor by a public index map: y[o] = x[idx[o]], 0 <= idx[o] < Nin (repeats allowed,
// inputs may go unread); od: the output dims, their product is idx's length
struct GatherGeom {
    const std::vector<i64>* idx;
    const std::vector<i64>* od;
    GatherGeom(const Params& p, i64 Nin);
    i64 out_size() const { return static_cast<i64>(idx->size()); }
    i64 src(i64 o) const { return (*idx)[static_cast<size_t>(o)]; }
};

// Separable two-tap interpolation of a (C, H, W) tensor by public tables (bilinear Resize, docs/BILINEAR.md):
//   y[c][oy][ox] = sum_{a, b in {0, 1}} wy_a[oy] wx_b[ox] x[c][y_a[oy]][x_b[ox]],
// wy_1 = ny[oy] in [0, 2^by], wy_0 = 2^by - ny[oy], likewise in x: 2^(by + bx) times the interpolated value. The
// tables are taken as they are (the coordinate modes exist in the IR only); by, bx <= 8.
struct BilinearGeom {
    static constexpr i64 kMaxBits = 8;
    i64 C, H, W, OH, OW, by, bx;
    const std::vector<i64>*y0, *y1, *ny, *x0, *x1, *nx;
    explicit BilinearGeom(const Params& p);
    i64 in_size() const { return C * H * W; }
    i64 out_size() const { return C * OH * OW; }
    // the two row / column weights of an output row / column, reduced mod p
    i64 wy(i64 oy, int a, i64 p) const {
        const i64 n = (*ny)[static_cast<size_t>(oy)];
        return (a ? n : (i64(1) << by) - n) % p;
    }
    i64 wx(i64 ox, int a, i64 p) const {
        const i64 n = (*nx)[static_cast<size_t>(ox)];
        return (a ? n : (i64(1) << bx) - n) % p;
    }
};
// the layer's map on labels of any moduli: out = sum of (weight mod p) * tap per residue (zero weights add nothing)
CrtLabels bilinear_labels(const BilinearGeom& G, const CrtLabels& cur, int nt);

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
