// MatMul layer kernels for gfx950 (gadgets.h MatMulPlan; kargs.h MatMulArgs; docs/MATMUL.md), a lane form
// (k_matmul) and a blocked form (k_matmul_b) between which the planner chooses: the contraction of
// two secret tensors, out[i, l] = sum_t x[i, t] y[t, l], as T generalized half gates per output element and
// residue whose product labels never leave the chip.
//
// Hardened only: no AES prologue. Both pads of a product are ChaCha pads (hard_pad) derived here from the two
// operands' compressed labels under the product's gate, rows (TW_MMG, j) of x and (TW_GME, j) of y. The key
// pre-pass (launch_label_key) compressed every element of x and y once; the multiply reads 16 bytes and a colour
// per operand and product, never the label columns: the digits of x are the base-p digits of its compressed label.
#include "gadget_walks.h"

namespace dash {
namespace dev {

constexpr int kMmBS = 256;

// What a lane needs of product t: gathered one product ahead, so the table rows are in flight under the pads
struct MatMulOps {
    u128 Kx, Ky, Graw, Eraw;
    uint32_t coly;
};
__device__ __forceinline__ MatMulOps matmul_ops(const MatMulArgs& a, const u128* kx, const uint16_t* cx, const u128* ky,
                                                const uint16_t* cy, int64_t row, int64_t t) {
    MatMulOps r;
    const uint32_t colx = cx[t * a.xst];
    r.coly = cy[t * a.yst];
    const int64_t rt = row + t * a.crt.sum;
    r.Graw = a.g[rt + colx];
    r.Eraw = a.e[rt + r.coly];
    r.Kx = kx[t * a.xst];
    r.Ky = ky[t * a.yst];
    return r;
}

// A lane's finished column: the bits of W (p = 2) or its column of the accumulator image, written once
__device__ __forceinline__ void matmul_store(act_t* Y, int64_t No, int n, const ModC& m, u128 W, const uint8_t* col) {
    if (m.bits == 1) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t ww = static_cast<uint32_t>(W >> (32 * w));
#pragma unroll 8
            for (int u = 0; u < 32; ++u) {
                const int d = 32 * w + u;
                if (d >= n) break;
                Y[static_cast<int64_t>(d) * No] = static_cast<act_t>((ww >> u) & 1u);
            }
        }
    } else {
        for (int d = 0; d < n; ++d) Y[static_cast<int64_t>(d) * No] = col[d * kMmBS];
    }
}

// The lane form: a lane owns output element o = i N + l of residue j and GC b, walks t and accumulates the digits
// E + colour(y) x - G of every product: p = 2 as bit logic on one 128-bit word in registers (the compressed label
// of x is its bits), every other residue in the lane's own column of an LDS image of kMmBS-byte rows, one byte
// per digit, reduced at every step. The finished column is written once. Lanes never read each other's columns:
// no barrier. grid (ceil(G M N / kMmBS), k, B), dynamic LDS a.lds_n * kMmBS bytes.
// kHeads (a.G > 1): the lanes run over the flat G M N outputs, a lane derives its head and offsets its operand bases
// by the head's slabs; a wave may straddle a head boundary. The table row and e0 follow o in both instantiations, and
// the single-head one compiles as it did before heads existed.
template <bool kHeads>
__global__ __launch_bounds__(kMmBS) void k_matmul(MatMulArgs a, Act y, const ModC* mc) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mm_acc[];
    const int j = blockIdx.y, b = blockIdx.z;
    const int tid = static_cast<int>(threadIdx.x);
    const int64_t Nh = a.M * a.N;  // outputs per head
    const int64_t No = kHeads ? a.G * Nh : Nh;
    const int64_t o = static_cast<int64_t>(blockIdx.x) * kMmBS + tid;
    if (o >= No) return;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const int64_t hg = kHeads ? o / Nh : 0, oh = o - hg * Nh;
    const int64_t i = oh / a.N, l = oh - i * a.N;
    const int64_t bk = static_cast<int64_t>(b) * a.crt.k + j;
    const int64_t nx = a.M * a.T, ny = a.T * a.N;  // a head's slabs
    const int64_t xb = (kHeads ? bk * a.G + hg : bk) * nx + i * a.xsi;
    const int64_t yb = (kHeads ? bk * a.G + hg : bk) * ny + l * a.ysl;
    const u128* kx = a.kx + xb;
    const uint16_t* cx = a.cx + xb;
    const u128* ky = a.ky + yb;
    const uint16_t* cy = a.cy + yb;
    const int64_t row = (static_cast<int64_t>(b) * No + o) * a.T * a.crt.sum + a.crt.prefix[j];
    const uint64_t e0 = static_cast<uint64_t>(o) * static_cast<uint64_t>(a.T);
    uint8_t* col = mm_acc + tid;
    u128 W = 0;
    MatMulOps nxt = matmul_ops(a, kx, cx, ky, cy, row, 0);
    for (int64_t t = 0; t < a.T; ++t) {
        const MatMulOps c = nxt;
        if (t + 1 < a.T) nxt = matmul_ops(a, kx, cx, ky, cy, row, t + 1);
        const uint64_t gt = a.gate0 ^ (e0 + static_cast<uint64_t>(t));
        u128 G = c.Graw - hard_pad(c.Kx, gt, tw_sub(kTwMmg, j), 0);
        u128 E = c.Eraw - hard_pad(c.Ky, gt, tw_sub(kTwGme, j), 0);
        const bool first = t == 0;
        if (m.bits == 1) {
            W ^= G ^ E ^ (c.coly ? c.Kx : static_cast<u128>(0));
        } else if (m.bits) {
            DigitStream sg, se, sx;
            sg.init(G);
            se.init(E);
            sx.init(c.Kx);
            for (int d = 0; d < n; ++d) {
                const uint32_t g = sg.next(m);
                const uint32_t ev = se.next(m) + (first ? 0u : static_cast<uint32_t>(col[d * kMmBS]));
                col[d * kMmBS] = static_cast<uint8_t>(mult_digit(ev, c.coly, sx.next(m), p, g, m));
            }
        } else {
            // chunk-major (chunk_digit): one divmod per stream per chunk; ev + acc + ypr x + p - g < p^2 + 3p
            u128 X = c.Kx;
            const int ch = static_cast<int>(m.c);
            for (int k0 = 0; k0 < n; k0 += ch) {
                uint32_t rg = divmod128(G, m), re = divmod128(E, m), rx = divmod128(X, m);
                const int kc = min(ch, n - k0);
#pragma unroll 4
                for (int u = 0; u < kc; ++u) {
                    const uint32_t g = chunk_digit(rg, m);
                    uint8_t& v = col[(k0 + u) * kMmBS];
                    const uint32_t ev = chunk_digit(re, m) + (first ? 0u : static_cast<uint32_t>(v));
                    v = static_cast<uint8_t>(mult_digit(ev, c.coly, chunk_digit(rx, m), p, g, m));
                }
            }
        }
    }
    matmul_store(y.p[j] + static_cast<int64_t>(b) * n * No + o, No, n, m, W, col);
}

// The blocked form: a block owns a kMmI x kMmL tile of outputs of residue j and GC b, lane (li, ll) output
// (i0 + li, l0 + ll). Per chunk of kMmTC products the block stages in LDS, once and through 16-byte loads, the
// compressed labels and colours of the tile's x rows (kMmI x kMmTC) and y columns (kMmTC x kMmL), one of each per
// lane, and the staging lane of an x element decompresses its digits into a column of a second image: the kMmL
// lanes of an output row share one x label's key, colour and digits (the lane form fetches the key and extracts the
// digits in every one of them), the kMmI lanes of an output column one y label's key and colour. Each lane streams
// its own output's contiguous table rows and accumulates as the lane form does. Lanes past the tile's edge stage
// and wait at the barriers but gather, hash and store nothing. grid (G tiles-per-head, k, B), dynamic LDS
// 2 a.lds_n kMmBS + 36 kMmBS bytes.
// kHeads (a.G > 1): blockIdx.x = head * tiles-per-head + tile, so a tile never spans heads; i0, l0, the edge tests
// and the staging indices are the head's own, against operand bases offset by the head's slabs, and a tile on a
// head's edge touches nothing of the next head.
template <bool kHeads>
__global__ __launch_bounds__(kMmBS) void k_matmul_b(MatMulArgs a, Act y, const ModC* mc) {
    static_assert(kMmI * kMmL == kMmBS && kMmI * kMmTC == kMmBS && kMmTC * kMmL == kMmBS, "one staged label per lane");
    extern __shared__ __attribute__((aligned(16))) uint8_t mm_lds[];
    const int j = blockIdx.y, b = blockIdx.z;
    const int tid = static_cast<int>(threadIdx.x);
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    uint8_t* col = mm_lds + tid;                                 // accumulator image [lds_n][kMmBS]
    uint8_t* xd = mm_lds + static_cast<size_t>(a.lds_n) * kMmBS;  // x digit image [lds_n][kMmBS], column = staging lane
    u128* kxs = reinterpret_cast<u128*>(mm_lds + 2 * static_cast<size_t>(a.lds_n) * kMmBS);
    u128* kys = kxs + kMmBS;
    uint16_t* cxs = reinterpret_cast<uint16_t*>(kys + kMmBS);
    uint16_t* cys = cxs + kMmBS;
    const int64_t tilesL = (a.N + kMmL - 1) / kMmL;
    const int64_t tilesH = kHeads ? ((a.M + kMmI - 1) / kMmI) * tilesL : 0;  // tiles per head
    const int64_t hg = kHeads ? static_cast<int64_t>(blockIdx.x) / tilesH : 0;
    const int64_t tile = static_cast<int64_t>(blockIdx.x) - hg * tilesH;
    const int64_t i0 = (tile / tilesL) * kMmI;
    const int64_t l0 = (tile % tilesL) * kMmL;
    const int li = tid / kMmL, ll = tid % kMmL;
    const bool live = i0 + li < a.M && l0 + ll < a.N;
    const int64_t No = kHeads ? a.G * a.M * a.N : a.M * a.N;
    const int64_t o = live ? (hg * a.M + i0 + li) * a.N + l0 + ll : 0;
    const int64_t bk = static_cast<int64_t>(b) * a.crt.k + j;
    const int64_t xb = (kHeads ? bk * a.G + hg : bk) * (a.M * a.T);
    const int64_t yb = (kHeads ? bk * a.G + hg : bk) * (a.T * a.N);
    const u128* kx = a.kx + xb;
    const uint16_t* cx = a.cx + xb;
    const u128* ky = a.ky + yb;
    const uint16_t* cy = a.cy + yb;
    const int64_t row = (static_cast<int64_t>(b) * No + o) * a.T * a.crt.sum + a.crt.prefix[j];
    const uint64_t e0 = static_cast<uint64_t>(o) * static_cast<uint64_t>(a.T);
    const int sxi = tid / kMmTC, sxt = tid % kMmTC;  // this lane stages x[i0 + sxi, t0 + sxt]
    const int syt = tid / kMmL, syl = tid % kMmL;    // and y[t0 + syt, l0 + syl]
    u128 W = 0;
    for (int64_t t0 = 0; t0 < a.T; t0 += kMmTC) {
        const int tc = static_cast<int>(min(static_cast<int64_t>(kMmTC), a.T - t0));
        __syncthreads();  // the previous chunk's products have read the images
        if (i0 + sxi < a.M && sxt < tc) {
            const int64_t ix = (i0 + sxi) * a.xsi + (t0 + sxt) * a.xst;
            u128 X = kx[ix];
            kxs[tid] = X;
            cxs[tid] = cx[ix];
            if (m.bits > 1) {
                DigitStream sx;
                sx.init(X);
                for (int d = 0; d < n; ++d) xd[d * kMmBS + tid] = static_cast<uint8_t>(sx.next(m));
            } else if (!m.bits) {
                const int ch = static_cast<int>(m.c);
                for (int k0 = 0; k0 < n; k0 += ch) {
                    uint32_t rx = divmod128(X, m);
                    const int kc = min(ch, n - k0);
                    for (int u = 0; u < kc; ++u) xd[(k0 + u) * kMmBS + tid] = static_cast<uint8_t>(chunk_digit(rx, m));
                }
            }
        }
        if (l0 + syl < a.N && syt < tc) {
            const int64_t iy = (t0 + syt) * a.yst + (l0 + syl) * a.ysl;
            kys[tid] = ky[iy];
            cys[tid] = cy[iy];
        }
        __syncthreads();
        if (!live) continue;
        for (int tt = 0; tt < tc; ++tt) {
            const int64_t t = t0 + tt;
            const int sx = li * kMmTC + tt, sy = tt * kMmL + ll;
            const uint32_t colx = cxs[sx], coly = cys[sy];
            const int64_t rt = row + t * a.crt.sum;
            const u128 Graw = a.g[rt + colx], Eraw = a.e[rt + coly];
            const u128 Kx = kxs[sx];
            const uint64_t gt = a.gate0 ^ (e0 + static_cast<uint64_t>(t));
            u128 G = Graw - hard_pad(Kx, gt, tw_sub(kTwMmg, j), 0);
            u128 E = Eraw - hard_pad(kys[sy], gt, tw_sub(kTwGme, j), 0);
            const bool first = t == 0;
            const uint8_t* xc = xd + sx;
            if (m.bits == 1) {
                W ^= G ^ E ^ (coly ? Kx : static_cast<u128>(0));
            } else if (m.bits) {
                DigitStream sg, se;
                sg.init(G);
                se.init(E);
                for (int d = 0; d < n; ++d) {
                    const uint32_t g = sg.next(m);
                    const uint32_t ev = se.next(m) + (first ? 0u : static_cast<uint32_t>(col[d * kMmBS]));
                    col[d * kMmBS] = static_cast<uint8_t>(mult_digit(ev, coly, xc[d * kMmBS], p, g, m));
                }
            } else {
                const int ch = static_cast<int>(m.c);
                for (int k0 = 0; k0 < n; k0 += ch) {
                    uint32_t rg = divmod128(G, m), re = divmod128(E, m);
                    const int kc = min(ch, n - k0);
#pragma unroll 4
                    for (int u = 0; u < kc; ++u) {
                        const uint32_t g = chunk_digit(rg, m);
                        uint8_t& v = col[(k0 + u) * kMmBS];
                        const uint32_t ev = chunk_digit(re, m) + (first ? 0u : static_cast<uint32_t>(v));
                        v = static_cast<uint8_t>(mult_digit(ev, coly, xc[(k0 + u) * kMmBS], p, g, m));
                    }
                }
            }
        }
    }
    if (!live) return;
    matmul_store(y.p[j] + static_cast<int64_t>(b) * n * No + o, No, n, m, W, col);
}

void launch_matmul(const MatMulArgs& a, const Act& y, int B, const ModC* mc, hipStream_t st) {
    const int64_t No = a.G * a.M * a.N;
    const bool heads = a.G > 1;
    if (a.blocked) {
        const int64_t tiles = a.G * ((a.M + kMmI - 1) / kMmI) * ((a.N + kMmL - 1) / kMmL);
        const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(a.crt.k), static_cast<unsigned>(B));
        if (launch_log_on()) launch_log_add("matmul.blocked", grid, dim3(kMmBS));
        // 49 KiB at k = 7: above the default dynamic LDS limit of a kernel (raised once, as for the staged chain)
        static const bool raised = [] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_matmul_b<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 64 << 10) == hipSuccess &&
                   hipFuncSetAttribute(reinterpret_cast<const void*>(&k_matmul_b<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 64 << 10) == hipSuccess;
        }();
        (void)raised;
        const size_t lds = (2 * static_cast<size_t>(a.lds_n) + 36) * kMmBS;
        if (heads) hipLaunchKernelGGL(k_matmul_b<true>, grid, dim3(kMmBS), lds, st, a, y, mc);
        else hipLaunchKernelGGL(k_matmul_b<false>, grid, dim3(kMmBS), lds, st, a, y, mc);
        return;
    }
    const dim3 grid(static_cast<unsigned>((No + kMmBS - 1) / kMmBS), static_cast<unsigned>(a.crt.k),
                    static_cast<unsigned>(B));
    if (launch_log_on()) launch_log_add("matmul.lane", grid, dim3(kMmBS));
    const size_t lds = static_cast<size_t>(a.lds_n) * kMmBS;
    if (heads) hipLaunchKernelGGL(k_matmul<true>, grid, dim3(kMmBS), lds, st, a, y, mc);
    else hipLaunchKernelGGL(k_matmul<false>, grid, dim3(kMmBS), lds, st, a, y, mc);
}

}  // namespace dev
}  // namespace dash
