// Gadget kernels for gfx950: approximate sign (3 phases), ReLU multiply,
// rescale (legacy sign-BE and ReDash base extension), projection and
// multiplication test gates.
//
// Work decomposition (vs the reference's one-stream-per-residue launches,
// sign_gadget.h:737-795, garbled_relu.h:258-294):
//   phase A  one lane per (GC, residue, element): ONE hash per input label,
//            reused for all |mrs| approx projections and later for the ReLU
//            garbler half-gate (the reference hashes the same key |mrs|+1
//            times); outputs stay compressed (u128).
//   phase B  one lane per (GC, element): the serial mixed-radix carry chain,
//            fully in registers, no device malloc (reference uses new[]).
//   phase C  one lane per (GC, residue, element): ReLU mixed-mod multiply, no
//            AES at all (hashes come from phases A/B).
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "gadget_walks.h"

namespace dash {
namespace dev {


// ---------------------------------------------------------------------------
// Phase A tail: the casts Z_{m_d} -> Z_{(k+1) m_d} of residue j's approx
// labels for every digit d >= 1. They do not depend on the carry, so they run
// here, in the lane that just produced the approx labels (still in registers):
// all cast gathers are issued before the paired AES. mrsP[b][j][d] receives
// the approx label for d = 0 and its cast for d >= 1 (phase B1 only sums).
// P[d] = approx label of digit d for d < TM; digits >= TM (t > TM) are
// recomputed from the approx row TA at color `col` (key H).
template <int TM>
__device__ __forceinline__ void approx_casts_out(const AesCtx& aes, const SignArgs& a, const ModC* mc, int j, int b,
                                                 int64_t e, const u128 (&P)[TM], const u128* TA, uint32_t col, u128 H) {
    const int64_t N = a.N;
    const int t = a.t;
    u128* out = a.mrsP + (static_cast<int64_t>(b) * a.crt.k + j) * t * N + e;
    if (a.fused) {
        // fused construction: the approx row already holds every digit in its summation modulus
#pragma unroll
        for (int d = 0; d < TM; ++d)
            if (d < t) out[static_cast<int64_t>(d) * N] = P[d];
        for (int d = TM; d < t; ++d) out[static_cast<int64_t>(d) * N] = TA[col * t + d] - H;
        return;
    }
    const u128* T1 = a.cast1 + (static_cast<int64_t>(b) * N + e) * a.n_cast;
    out[0] = P[0];
    u128 tt[TM];
#pragma unroll
    for (int d = 1; d < TM; ++d)
        if (d < t) {
            const int m = a.mrs[d];
            tt[d] = T1[a.c1off[d] + static_cast<int64_t>(j) * m + u128_mod(P[d], mc[m])];
        }
#pragma unroll
    for (int d = 1; d < TM; d += 2) {
        if (d < t) {
            const bool two = (d + 1 < TM) && (d + 1 < t);
            const u128 PB = (d + 1 < TM) ? P[(d + 1 < TM) ? d + 1 : d] : static_cast<u128>(0);
            u128 HA, HB = 0;
            if (two)
                aes_encrypt2(aes, P[d], PB, HA, HB);
            else
                HA = aes_encrypt(aes, P[d]);
            out[static_cast<int64_t>(d) * N] = tt[d] - HA;
            if (two) out[static_cast<int64_t>(d + 1) * N] = tt[(d + 1 < TM) ? d + 1 : d] - HB;
        }
    }
    for (int d = TM; d < t; ++d) {
        const int m = a.mrs[d];
        const u128 Pd = TA[col * t + d] - H;
        const u128 Td = T1[a.c1off[d] + static_cast<int64_t>(j) * m + u128_mod(Pd, mc[m])];
        out[static_cast<int64_t>(d) * N] = Td - aes_encrypt(aes, Pd);
    }
}

// Phase A: approximate residues + their casts. grid (x, k, B)
template <int TM>
__global__ __launch_bounds__(kAesBlock, kSignApproxMinWaves) void k_sign_approx(SignArgs a, Act x, const ModC* mc, const uint32_t* te0,
                                                     const uint32_t* rk) {
    AES_PROLOGUE(te0, rk);
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int p = a.crt.p[j];
        const ModC m = mc[p];
        const act_t* L = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
        const uint32_t col = static_cast<uint16_t>(L[0]) % static_cast<uint32_t>(p);
        const u128* T =
            a.approx + (static_cast<int64_t>(b) * N + e) * a.n_approx + static_cast<int64_t>(a.t) * a.crt.prefix[j];
        // issue the table gathers first: their HBM latency hides under the AES
        u128 P[TM];
#pragma unroll
        for (int d = 0; d < TM; ++d)
            if (d < a.t) P[d] = T[col * a.t + d];
        const u128 C = compress_cm<kSignApproxChunk>(L, N, m);
        const int64_t bke = (static_cast<int64_t>(b) * a.crt.k + j) * N + e;
        if (a.hard) {
            // hardened (fused only): digit d's entry under pad d of (C, sign gate, (TW_APPROX, j)); the ReLU's garbler
            // half gate keyed by the same label gets its own pad (mixed-mult gate, (TW_MMG, j))
            const uint64_t sg = a.sgate0 ^ static_cast<uint64_t>(e);
            u128* out = a.mrsP + (static_cast<int64_t>(b) * a.crt.k + j) * a.t * N + e;
            for (int blk = 0; 4 * blk < a.t; ++blk) {
                u128 pd[4];
                hard_block(C, sg, tw_sub(kTwApprox, j), static_cast<uint32_t>(blk), pd);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int d = 4 * blk + q;
                    if (d < a.t) out[static_cast<int64_t>(d) * N] = T[col * a.t + d] - pd[q];
                }
            }
            if (a.hx) {
                a.hx[bke] = hard_pad(C, a.mgate0 ^ static_cast<uint64_t>(e), tw_sub(kTwMmg, j), 0);
                a.colx[bke] = static_cast<uint16_t>(col);
            }
            continue;
        }
        const u128 H = aes_encrypt(aes, C);
        if (a.hx) {
            a.hx[bke] = H;
            a.colx[bke] = static_cast<uint16_t>(col);
        }
#pragma unroll
        for (int d = 0; d < TM; ++d)
            if (d < a.t) P[d] -= H;
        approx_casts_out<TM>(aes, a, mc, j, b, e, P, T, col, H);
    }
}

// ---------------------------------------------------------------------------
// Phase B1: per MRS digit, the component-wise sum over residues j of the
// phase-A outputs (casts mod (k+1) m_d for d >= 1, approx labels mod m_0 for
// d = 0). No AES and no LDS, so it runs at full occupancy.
// grid (ceil(N/256), t, B): blockIdx.y = t-1 is digit 0, otherwise digit y+1.
template <int MAXN>
__global__ __launch_bounds__(256) void k_sign_castsum(SignArgs a, const ModC* mc) {
    const int b = blockIdx.z;
    const int k = a.crt.k, t = a.t;
    const int d = (static_cast<int>(blockIdx.y) == t - 1) ? 0 : static_cast<int>(blockIdx.y) + 1;
    const int64_t N = a.N;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int m = a.mrs[d];
    const int mo = d ? (k + 1) * m : m;
    const ModC Mo = mc[mo];
    const u128* P0 = a.mrsP + (static_cast<int64_t>(b) * k * t + d) * N + e;
    int32_t acc[MAXN];
#pragma unroll
    for (int i = 0; i < MAXN; ++i) acc[i] = 0;
    u128 nk = P0[0];
    for (int j = 0; j < k; ++j) {
        DigitStream s;
        s.init(nk);
        if (j + 1 < k) nk = P0[static_cast<int64_t>(j + 1) * t * N];
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
            if (i < static_cast<int>(Mo.n)) acc[i] += static_cast<int32_t>(s.next(Mo));
    }
    int16_t* S = a.csum + ((static_cast<int64_t>(b) * t + d) * kCsumComps) * N + e;
#pragma unroll
    for (int i = 0; i < MAXN; ++i)
        if (i < static_cast<int>(Mo.n)) S[i * N] = static_cast<int16_t>(modq(static_cast<uint32_t>(acc[i]), Mo));
}

// ---------------------------------------------------------------------------
// Phase B2: the serial mixed-radix carry chain + sign projection. Per digit
// only the carry's cast and the sum's cast2 projection remain on the
// critical path (2 AES + 2 gathers). grid (x, 1, B)
template <int MAXN>
__global__ __launch_bounds__(kAesBlock, kAesMinBlocks) void k_sign_chain(SignArgs a, const ModC* mc, const uint32_t* te0,
                                                    const uint32_t* rk) {
    AES_PROLOGUE(te0, rk);
    const int b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k, t = a.t;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const u128* T1 = a.cast1 + (static_cast<int64_t>(b) * N + e) * a.n_cast;
        const u128* T2 = a.cast2 + (static_cast<int64_t>(b) * N + e) * a.n_cast;
        const int16_t* S = a.csum + static_cast<int64_t>(b) * t * kCsumComps * N + e;
        const int mlast = a.mrs[t - 1];
        u128 carry = a.zc[static_cast<int64_t>(b) * a.zc_stride + mlast];
        uint32_t ccol = a.zcol[static_cast<int64_t>(b) * a.zc_stride + mlast];
        int64_t c1 = 0, c2 = 0;
        int32_t acc[MAXN];
        for (int d = t - 1; d >= 1; --d) {
            const int m = a.mrs[d];
            const int mo = (k + 1) * m;
            const ModC Mo = mc[mo];
            const u128 TA = T1[c1 + static_cast<int64_t>(k) * m + ccol];
            const int16_t* Sd = S + static_cast<int64_t>(d) * kCsumComps * N;
#pragma unroll
            for (int i = 0; i < MAXN; ++i)
                if (i < static_cast<int>(Mo.n)) acc[i] = Sd[i * N];
            const u128 HA = aes_encrypt(aes, carry);
            c1 += static_cast<int64_t>(k + 1) * m;
            DigitStream sa;
            sa.init(TA - HA);
            CompressFwd cf;
            cf.init();
            uint32_t col2 = 0;
#pragma unroll
            for (int i = 0; i < MAXN; ++i)
                if (i < static_cast<int>(Mo.n)) {
                    uint32_t v = static_cast<uint32_t>(acc[i]) + sa.next(Mo);
                    if (v >= static_cast<uint32_t>(mo)) v -= mo;
                    if (i == 0) col2 = v;
                    cf.push(v, Mo);
                }
            const u128 key2 = cf.finish();
            const u128 T2e = T2[c2 + col2];
            const u128 H2 = aes_encrypt(aes, key2);
            carry = T2e - H2;
            c2 += mo;
            ccol = u128_mod(carry, mc[a.mrs[d - 1]]);
        }
        // most significant digit: sum = carry + sum_j mrs[j][0] (the latter from phase B1)
        const int m0 = a.mrs[0];
        const ModC M0 = mc[m0];
        DigitStream sc;
        sc.init(carry);
        CompressFwd cf;
        cf.init();
        uint32_t col = 0;
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
            if (i < static_cast<int>(M0.n)) {
                uint32_t v = static_cast<uint32_t>(S[i * N]) + sc.next(M0);
                if (v >= static_cast<uint32_t>(m0)) v -= m0;
                if (i == 0) col = v;
                cf.push(v, M0);
            }
        const u128 key = cf.finish();
        const u128* TS = a.sign + (static_cast<int64_t>(b) * N + e) * a.n_sign;
        const u128 TS0 = TS[col];
        const u128 H = aes_encrypt(aes, key);
        for (int o = 0; o < a.nout; ++o) {
            const u128 P = (o == 0 ? TS0 : TS[o * m0 + col]) - H;
            a.outP[(static_cast<int64_t>(b) * a.nout + o) * N + e] = P;
            if (a.relu && o == 0) {
                a.hs[static_cast<int64_t>(b) * N + e] = aes_encrypt(aes, P);
                a.cs[static_cast<int64_t>(b) * N + e] = static_cast<uint8_t>(static_cast<uint32_t>(P) & 1u);
            }
        }
    }
}

// Phase B2 of the fused construction (SignPlan::fused): the carry leaves each
// carry projection already in the next digit's summation modulus, so a digit
// costs ONE dependent gather + ONE AES on the critical path (the reference
// construction: two of each). The least significant digit has no carry-in.
// grid (x, 1, B)
template <int MAXN>
__global__ __launch_bounds__(kAesBlock, kAesMinBlocks) void k_sign_chain_fused(SignArgs a, const ModC* mc,
                                                                               const uint32_t* te0, const uint32_t* rk) {
    AES_PROLOGUE(te0, rk);
    const int b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k, t = a.t;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const u128* T2 = a.cast2 + (static_cast<int64_t>(b) * N + e) * a.n_cast;
        const int16_t* S = a.csum + static_cast<int64_t>(b) * t * kCsumComps * N + e;
        u128 carry = 0;
        int64_t c2 = 0;
        int32_t acc[MAXN];
        for (int d = t - 1; d >= 1; --d) {
            const int mo = (k + 1) * a.mrs[d];
            const ModC Mo = mc[mo];
            const int16_t* Sd = S + static_cast<int64_t>(d) * kCsumComps * N;
#pragma unroll
            for (int i = 0; i < MAXN; ++i)
                if (i < static_cast<int>(Mo.n)) acc[i] = Sd[i * N];
            const bool have = d < t - 1;
            DigitStream sa;
            sa.init(carry);
            CompressFwd cf;
            cf.init();
            uint32_t col2 = 0;
#pragma unroll
            for (int i = 0; i < MAXN; ++i)
                if (i < static_cast<int>(Mo.n)) {
                    uint32_t v = static_cast<uint32_t>(acc[i]);
                    if (have) {
                        v += sa.next(Mo);
                        if (v >= static_cast<uint32_t>(mo)) v -= mo;
                    }
                    if (i == 0) col2 = v;
                    cf.push(v, Mo);
                }
            const u128 key2 = cf.finish();
            const u128 T2e = T2[c2 + col2];
            carry = T2e - (a.hard ? hard_pad(key2, a.sgate0 ^ static_cast<uint64_t>(e), tw_sub(kTwCast2, d), 0)
                                  : aes_encrypt(aes, key2));
            c2 += mo;
        }
        const int m0 = a.mrs[0];
        const ModC M0 = mc[m0];
        const bool have = t >= 2;
        DigitStream sc;
        sc.init(carry);
        CompressFwd cf;
        cf.init();
        uint32_t col = 0;
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
            if (i < static_cast<int>(M0.n)) {
                uint32_t v = static_cast<uint32_t>(S[i * N]);
                if (have) {
                    v += sc.next(M0);
                    if (v >= static_cast<uint32_t>(m0)) v -= m0;
                }
                if (i == 0) col = v;
                cf.push(v, M0);
            }
        const u128 key = cf.finish();
        const u128* TS = a.sign + (static_cast<int64_t>(b) * N + e) * a.n_sign;
        const u128 TS0 = TS[col];
        const u128 H = a.hard ? 0 : aes_encrypt(aes, key);
        const uint64_t sg = a.sgate0 ^ static_cast<uint64_t>(e);
        for (int o = 0; o < a.nout; ++o) {
            const u128 P = (o == 0 ? TS0 : TS[o * m0 + col]) - (a.hard ? hard_pad(key, sg, tw_sub(kTwSign, 0), o) : H);
            a.outP[(static_cast<int64_t>(b) * a.nout + o) * N + e] = P;
            if (a.relu && o == 0) {
                if (a.hard) {  // the sign label's y-row pads (ReLU evaluator half gates + minis)
                    const uint64_t mg = a.mgate0 ^ static_cast<uint64_t>(e);
                    for (int blk = 0; 4 * blk < a.ny; ++blk) {
                        u128 pd[4];
                        hard_block(P, mg, tw_sub(kTwMmy, 0), static_cast<uint32_t>(blk), pd);
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (4 * blk + q < a.ny) a.ys[(static_cast<int64_t>(b) * a.ny + 4 * blk + q) * N + e] = pd[q];
                    }
                } else {
                    a.hs[static_cast<int64_t>(b) * N + e] = aes_encrypt(aes, P);
                }
                a.cs[static_cast<int64_t>(b) * N + e] = static_cast<uint8_t>(static_cast<uint32_t>(P) & 1u);
            }
        }
    }
}

// Decompress compressed outputs into residue activations. grid (ceil(N/256), nres, B)
__global__ __launch_bounds__(256) void k_unpack(const u128* P, int nres, Act out, CrtInfo mods, const ModC* mc,
                                                int64_t N) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const ModC m = mc[mods.p[j]];
    DigitStream s;
    s.init(P[(static_cast<int64_t>(b) * nres + j) * N + e]);
    act_t* o = out.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    for (int i = 0; i < static_cast<int>(m.n); ++i) o[i * N] = static_cast<act_t>(s.next(m));
}

// ---------------------------------------------------------------------------
// Phase C: ReLU = x * sign01(x) via the mixed-modulus half gate.
// grid (ceil(N/256), k, B)
__global__ __launch_bounds__(256) void k_relu_mult(SignArgs a, Act x, Act y, const u128* gtab, const u128* etab,
                                                   const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int k = a.crt.k;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + e;
    const u128 Hx = a.hx[bke];
    const uint32_t colx = a.colx[bke];
    const int64_t be = static_cast<int64_t>(b) * N + e;
    const ReluOps o = relu_ops(a.hard ? nullptr : a.hs, a.ys, a.ny, a.cs, etab, b, j, k, N, e);
    const u128 G = gtab[be * a.crt.sum + a.crt.prefix[j] + colx] - Hx;
    const uint32_t ypr = mini_mult(o.mini, o.cS, o.HM, p, m);
    DigitStream sg, se;
    sg.init(G);
    se.init(o.Eraw - o.HS);
    col_walk<kChunk>(x.p[j] + static_cast<int64_t>(b) * m.n * N + e, y.p[j] + static_cast<int64_t>(b) * m.n * N + e, N,
                     static_cast<int>(m.n), [&](int, uint32_t xv) {
                         const uint32_t g = sg.next(m);
                         return mult_digit(se.next(m), ypr, xv, p, g, m);
                     });
}

// k_relu_mult with the label staged in LDS (stage_ok): a block = (256-element tile, residue j, GC b); the
// per-element gathers go out first, the block's x_j rows come in as 16-byte loads, each lane rewrites its
// column in place and the block stores the y_j rows back as 16-byte stores.
constexpr int kRmBS = 256;
__global__ __launch_bounds__(kRmBS) void k_relu_mult_s(SignArgs a, Act x, Act y, const u128* gtab, const u128* etab,
                                                       const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[128 * kRmBS];
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int tid = static_cast<int>(threadIdx.x);
    const int k = a.crt.k;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * n * N;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * n * N;
    for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRmBS; e0 < N; e0 += static_cast<int64_t>(gridDim.x) * kRmBS) {
        const int64_t e = min(e0 + tid, N - 1);
        const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + e;
        const int64_t be = static_cast<int64_t>(b) * N + e;
        const u128 Hx = a.hx[bke];
        const uint32_t colx = a.colx[bke];
        const ReluOps o = relu_ops(a.hard ? nullptr : a.hs, a.ys, a.ny, a.cs, etab, b, j, k, N, e);
        const u128 Graw = gtab[be * a.crt.sum + a.crt.prefix[j] + colx];
        __syncthreads();  // the previous tile's stores have read the image
        lds_stage_rows<kRmBS, 4>(stg, X, N, e0, 0, n);
        __syncthreads();
        lds_mult_walk<kRmBS, false>(stg + tid, n, Graw - Hx, o.Eraw - o.HS, 0, mini_mult(o.mini, o.cS, o.HM, p, m), p, m);
        __syncthreads();
        lds_store_rows<kRmBS>(Y, stg, N, e0, 0, n);
    }
}

// ---------------------------------------------------------------------------
// LeakyRelu multiply (gadgets.h LeakyPlan): leaky_j = b x_j + c relu_j per digit, the ReLU multiply's operands
// and walks with the leaky epilogue (gadget_walks.h leaky_digit; p = 2 as bit logic). b, c: one table read per
// lane. grid (ceil(N/256), k, B), as k_relu_mult.
__global__ __launch_bounds__(256) void k_leaky_mult(SignArgs a, LeakyTab lk, Act x, Act y, const u128* gtab,
                                                    const u128* etab, const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int k = a.crt.k;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + e;
    const u128 Hx = a.hx[bke];
    const uint32_t colx = a.colx[bke];
    const int64_t be = static_cast<int64_t>(b) * N + e;
    const LeakyLane ll = leaky_lane(lk, e, j, k);
    const ReluOps o = relu_ops(a.hard ? nullptr : a.hs, a.ys, a.ny, a.cs, etab, b, j, k, N, e);
    const u128 G = gtab[be * a.crt.sum + a.crt.prefix[j] + colx] - Hx;
    const uint32_t ypr = mini_mult(o.mini, o.cS, o.HM, p, m);
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    DigitStream sg, se;
    sg.init(G);
    se.init(o.Eraw - o.HS);
    if (m.bits == 1) {
        col_walk<kChunk>(X, Y, N, static_cast<int>(m.n), [&](int, uint32_t xv) {
            const uint32_t t = se.next(m) ^ sg.next(m) ^ (xv & ypr);
            return (ll.fb & xv) ^ (ll.fc & t);
        });
    } else {
        const uint32_t yl = leaky_mult(ypr, ll, m);
        col_walk<kChunk>(X, Y, N, static_cast<int>(m.n), [&](int, uint32_t xv) {
            const uint32_t g = sg.next(m);
            return leaky_digit(se.next(m), yl, xv, p, g, ll.fc, m);
        });
    }
}

// k_leaky_mult with the label staged in LDS (stage_ok), as k_relu_mult_s: a block = (256-element tile, residue j,
// GC b). A tile may span channels: every lane reads its own element's factors.
__global__ __launch_bounds__(kRmBS) void k_leaky_mult_s(SignArgs a, LeakyTab lk, Act x, Act y, const u128* gtab,
                                                        const u128* etab, const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[128 * kRmBS];
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int tid = static_cast<int>(threadIdx.x);
    const int k = a.crt.k;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * n * N;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * n * N;
    for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRmBS; e0 < N; e0 += static_cast<int64_t>(gridDim.x) * kRmBS) {
        const int64_t e = min(e0 + tid, N - 1);
        const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + e;
        const int64_t be = static_cast<int64_t>(b) * N + e;
        const u128 Hx = a.hx[bke];
        const uint32_t colx = a.colx[bke];
        const LeakyLane ll = leaky_lane(lk, e, j, k);
        const ReluOps o = relu_ops(a.hard ? nullptr : a.hs, a.ys, a.ny, a.cs, etab, b, j, k, N, e);
        const u128 Graw = gtab[be * a.crt.sum + a.crt.prefix[j] + colx];
        __syncthreads();  // the previous tile's stores have read the image
        lds_stage_rows<kRmBS, 4>(stg, X, N, e0, 0, n);
        __syncthreads();
        lds_mult_walk<kRmBS, false, true>(stg + tid, n, Graw - Hx, o.Eraw - o.HS, 0, mini_mult(o.mini, o.cS, o.HM, p, m),
                                          p, m, ll);
        __syncthreads();
        lds_store_rows<kRmBS>(Y, stg, N, e0, 0, n);
    }
}

// ---------------------------------------------------------------------------
// Clip multiply (gadgets.h ClipPlan): clip_j = E + ypr x_j - G + C, the ReLU multiply keyed by the label of
// u = s_lo + s_hi plus the cap row C of s_hi, from the two sign labels themselves. Mod-2 labels compress to
// their bit pack, so the compressed label of u is the XOR of the two sign labels; the lane derives u's
// y-row pads (TW_MMY, 0: entry slot j, mini lane j % 8 of slot k + j / 8) and the cap pad (TW_CAP, 0: slot j).
struct ClipLane {
    u128 G, E, C;
    uint32_t ypr;
};
// The rows keyed by the two sign labels (everything of a lane but the garbler half gate G, which hangs on the
// multiplied label's own key): shared by the clip multiply kernels and the fused rescale + clip output.
__device__ __forceinline__ ClipLane clip_keyed(const ClipArgs& a, int j, int b, int64_t e, int p, const ModC& m) {
    const int k = a.crt.k;
    const int64_t N = a.N;
    const int64_t be = static_cast<int64_t>(b) * N + e;
    // the gathers go out before the pads are computed
    const u128 Khi = a.khi[be];
    const u128 U = a.klo[be] ^ Khi;
    const uint32_t cH = static_cast<uint32_t>(Khi) & 1u;
    const u128 Craw = a.cap[(be * k + j) * 2 + cH];
    const uint64_t mg = a.mgate0 ^ static_cast<uint64_t>(e);
    const KeyedOps o = keyed_ops(U, mg, a.etab + (be * k + j) * 3, j, k, p, m);
    const u128 HC = hard_pad(Khi, mg, tw_sub(kTwCap, 0), j);
    ClipLane r;
    r.G = 0;
    r.E = o.E;
    r.C = Craw - HC;
    r.ypr = o.ypr;
    return r;
}
__device__ __forceinline__ ClipLane clip_lane(const ClipArgs& a, int j, int b, int64_t e, int p, const ModC& m) {
    const int64_t bke = (static_cast<int64_t>(b) * a.crt.k + j) * a.N + e;
    const u128 Hx = a.hx[bke];
    const uint32_t colx = a.colx[bke];
    const u128 Graw = a.gtab[(static_cast<int64_t>(b) * a.N + e) * a.crt.sum + a.crt.prefix[j] + colx];
    ClipLane r = clip_keyed(a, j, b, e, p, m);
    r.G = Graw - Hx;
    return r;
}

// grid (ceil(N/256), k, B)
__global__ __launch_bounds__(256) void k_clip_mult(ClipArgs a, Act x, Act y, const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const ClipLane c = clip_lane(a, j, b, e, p, m);
    DigitStream sg, se, sc;
    sg.init(c.G);
    se.init(c.E);
    sc.init(c.C);
    col_walk<kChunk>(x.p[j] + static_cast<int64_t>(b) * m.n * N + e, y.p[j] + static_cast<int64_t>(b) * m.n * N + e, N,
                     static_cast<int>(m.n), [&](int, uint32_t xv) {
                         const uint32_t g = sg.next(m);
                         const uint32_t ev = se.next(m);
                         return mult_digit(ev + sc.next(m), c.ypr, xv, p, g, m);
                     });
}

// k_clip_mult with the label staged in LDS (stage_ok; as k_relu_mult_s): a block = (256-element tile, residue
// j, GC b); the per-element gathers go out first, the block's x_j rows come in as 16-byte loads, each lane
// rewrites its column in place and the block stores the y_j rows back as 16-byte stores.
__global__ __launch_bounds__(kRmBS) void k_clip_mult_s(ClipArgs a, Act x, Act y, const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[128 * kRmBS];
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int tid = static_cast<int>(threadIdx.x);
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * n * N;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * n * N;
    for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRmBS; e0 < N; e0 += static_cast<int64_t>(gridDim.x) * kRmBS) {
        const int64_t e = min(e0 + tid, N - 1);  // lanes past the end redo the last element (their column is not stored)
        const ClipLane c = clip_lane(a, j, b, e, p, m);
        __syncthreads();  // the previous tile's stores have read the image
        lds_stage_rows<kRmBS, 4>(stg, X, N, e0, 0, n);
        __syncthreads();
        lds_mult_walk<kRmBS, true>(stg + tid, n, c.G, c.E, c.C, c.ypr, p, m);
        __syncthreads();
        lds_store_rows<kRmBS>(Y, stg, N, e0, 0, n);
    }
}

// ---------------------------------------------------------------------------
// PiecewiseLinear multiply (gadgets.h PwlPlan; kargs.h PwlArgs): out_j = a0 x_j + sum_i d_i relu_i,j with
// relu_i,j = E_i + ypr_i x_j - G_i, all M kept breakpoints' half gates in one pass over the label: it is read
// once and written once. Every breakpoint has its own gate, so the lane derives the (TW_MMG, j) pad of x_j and
// the y-row pads of the sign label (keyed_ops) per breakpoint from the compressed labels.
//
// kx[b][j][e] = compress(x_j), colx = colour (the pads are gate-dependent: no hash here). grid (x, k, B)
__global__ __launch_bounds__(256) void k_label_key(Act x, CrtInfo crt, int64_t N, u128* kx, uint16_t* colx,
                                                   const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const ModC m = mc[crt.p[j]];
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const act_t* L = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
        const int64_t bke = (static_cast<int64_t>(b) * crt.k + j) * N + e;
        colx[bke] = static_cast<uint16_t>(static_cast<uint16_t>(L[0]) % m.q);
        kx[bke] = compress_cm(L, N, m);
    }
}

template <int M>
__device__ __forceinline__ PwlLane<M> pwl_lane(const PwlArgs& a, int j, int b, int64_t e, int p, const ModC& m) {
    const int k = a.crt.k;
    const int64_t N = a.N;
    const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + e;
    const int64_t be = static_cast<int64_t>(b) * N + e;
    // the gathers go out before the pads are computed
    const u128 Kx = a.kx[bke];
    const uint32_t colx = a.colx[bke];
    u128 Ky[M], Graw[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        Ky[i] = a.key[i][be];
        Graw[i] = a.gtab[i][be * a.crt.sum + a.crt.prefix[j] + colx];
    }
    const uint8_t* f = a.fac + j * (M + 1);
    PwlLane<M> l;
    uint32_t ys = f[0];  // a0 + sum_i d_i ypr_i <= (p - 1) + M (p - 1)^2
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const uint64_t gate = a.mgate0[i] ^ static_cast<uint64_t>(e);
        const KeyedOps o = keyed_ops(Ky[i], gate, a.etab[i] + (be * k + j) * 3, j, k, p, m);
        l.G[i] = Graw[i] - hard_pad(Kx, gate, tw_sub(kTwMmg, j), 0);
        l.E[i] = o.E;
        l.d[i] = f[1 + i];
        ys += l.d[i] * o.ypr;
    }
    l.yl = modq(ys, m);
    return l;
}

// per-lane HBM column walk. grid (ceil(N/256), k, B)
template <int M>
__global__ __launch_bounds__(256) void k_pwl_mult(PwlArgs a, Act x, Act y, const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const PwlLane<M> l = pwl_lane<M>(a, j, b, e, p, m);
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    if (m.bits == 1) {
        DigitStream sw;
        sw.init(pwl_bit_word(l));
        const uint32_t yl = l.yl & 1u;
        col_walk<kChunk>(X, Y, N, static_cast<int>(m.n), [&](int, uint32_t xv) { return sw.next(m) ^ (xv & yl); });
    } else {
        DigitStream sg[M], se[M];
#pragma unroll
        for (int i = 0; i < M; ++i) {
            sg[i].init(l.G[i]);
            se[i].init(l.E[i]);
        }
        col_walk<kChunk>(X, Y, N, static_cast<int>(m.n), [&](int, uint32_t xv) {
            return pwl_digit(xv, l, p, m, [&](int i) { return sg[i].next(m); }, [&](int i) { return se[i].next(m); });
        });
    }
}

// k_pwl_mult with the label staged in LDS (stage_ok; as k_relu_mult_s): a block = (256-element tile, residue j,
// GC b). The units past the end of a partial last tile are staged as zeros, so its spare lanes (which redo the
// last element's operands) walk zero digits; their columns are not stored.
template <int M>
__global__ __launch_bounds__(kRmBS) void k_pwl_mult_s(PwlArgs a, Act x, Act y, const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[128 * kRmBS];
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int tid = static_cast<int>(threadIdx.x);
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * n * N;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * n * N;
    for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRmBS; e0 < N; e0 += static_cast<int64_t>(gridDim.x) * kRmBS) {
        const int64_t e = min(e0 + tid, N - 1);
        PwlLane<M> l = pwl_lane<M>(a, j, b, e, p, m);
        __syncthreads();  // the previous tile's stores have read the image
        lds_stage_rows<kRmBS, 4, true>(stg, X, N, e0, 0, n);
        __syncthreads();
        lds_pwl_walk<kRmBS, M>(stg + tid, n, l, p, m);
        __syncthreads();
        lds_store_rows<kRmBS>(Y, stg, N, e0, 0, n);
    }
}

// ---------------------------------------------------------------------------
// ArgMax (gadgets.h ArgMaxPlan; kargs.h ArgMaxArgs for the element layout).
// Pair differences of one level: d[e] = v[slot 2q] - v[slot 2q + 1], e = q P + o; the operation pubq has no b
// labels (a public index folded into the garbler's bases), its difference is a's label. grid (x, k, B)
__global__ __launch_bounds__(256) void k_argmax_diff(Act v, Act d, int64_t P, int ops, int cnt, int pubq, CrtInfo crt) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int n = crt.n[j], p = crt.p[j];
    const int64_t Nd = P * ops, Nv = P * cnt;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= Nd * n) return;
    const int64_t c = t / Nd, e = t - c * Nd, q = e / P;
    const act_t* V = v.p[j] + (static_cast<int64_t>(b) * n + c) * Nv + e + q * P;  // slot 2q of position o
    const int32_t x = static_cast<int32_t>(V[0]) - (q == pubq ? 0 : static_cast<int32_t>(V[P]));
    d.p[j][(static_cast<int64_t>(b) * n + c) * Nd + e] = static_cast<act_t>(x < 0 ? x + p : x);
}

// One half gate keyed by the sign label S: the garbler half's row of the multiplied label (its pad and colour
// from the hash pass) and the evaluator half's operands
struct ArgMaxGate {
    u128 G, E;
    uint32_t ypr;
};
__device__ __forceinline__ ArgMaxGate argmax_gate(const ArgMaxArgs& a, u128 S, uint64_t gate, const u128* hx,
                                                  const uint16_t* colx, const u128* gtab, const u128* etab, int j,
                                                  int64_t be, int64_t bke, int p, const ModC& m) {
    const u128 Hx = hx[bke];
    const uint32_t col = colx[bke];
    const u128 Graw = gtab[be * a.crt.sum + a.crt.prefix[j] + col];
    const KeyedOps o = keyed_ops(S, gate, etab + (be * a.crt.k + j) * 3, j, a.crt.k, p, m);
    ArgMaxGate r;
    r.G = Graw - Hx;
    r.E = o.E;
    r.ypr = o.ypr;
    return r;
}

// The multiply of one level, grid (ceil(N / 256), k, B), N = ops P: lane e fetches the sign label once, derives
// the pads of both gate sets, and writes v_b + s d and i_b + s e (level 0: the projection row of s) into slot q
// of the next level; the lanes of q = 0 also copy the carried slot. VAL: the level has value gates (not the
// root); L0: level 0 (public indices). d / ed: the pair differences; v / i: this level's candidates.
template <bool VAL, bool L0>
__global__ __launch_bounds__(256) void k_argmax_mult(ArgMaxArgs a, Act v, Act d, Act i, Act ed, Act nv, Act ni,
                                                     const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t P = a.P, N = P * a.ops, Nc = P * a.cnt, Nn = P * a.cnt1;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int k = a.crt.k, p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const int64_t q = e / P;
    const int64_t sb = e + (q + 1) * P;  // slot 2q + 1 of position o
    const int64_t be = static_cast<int64_t>(b) * N + e, bke = (static_cast<int64_t>(b) * k + j) * N + e;
    const int64_t gb = static_cast<int64_t>(b) * n;
    const u128 S = a.ks[be];
    ArgMaxGate gv{}, gi{};
    u128 C = 0;
    if (VAL) gv = argmax_gate(a, S, a.vgate0 ^ static_cast<uint64_t>(e), a.hx, a.colx, a.gtab, a.etab, j, be, bke, p, m);
    if (L0) {
        const u128 Craw = a.itab[(be * k + j) * 2 + (static_cast<uint32_t>(S) & 1u)];
        C = Craw - hard_pad(S, a.igate0 ^ static_cast<uint64_t>(e), tw_sub(kTwCap, 0), j);
    } else {
        gi = argmax_gate(a, S, a.igate0 ^ static_cast<uint64_t>(e), a.hi, a.coli, a.igtab, a.ietab, j, be, bke, p, m);
    }
    DigitStream svg, sve, sig, sie, sc;
    svg.init(gv.G);
    sve.init(gv.E);
    sig.init(gi.G);
    sie.init(gi.E);
    sc.init(C);
    const uint32_t up = static_cast<uint32_t>(p);
    const bool ib_secret = q != a.pubq;
    act_t* NV = nv.p[j] + gb * Nn + e;
    act_t* NI = ni.p[j] + gb * Nn + e;
    const act_t* Dj = d.p[j] + gb * N + e;
    const act_t* Vb = v.p[j] + gb * Nc + sb;
    // one digit of a gate's output plus the b candidate's digit, both in [0, p)
    auto gate_digit = [&](DigitStream& se, DigitStream& sg, uint32_t ypr, uint32_t x, uint32_t add) {
        const uint32_t g = sg.next(m);
        const uint32_t r = mult_digit(se.next(m), ypr, x, p, g, m) + add;
        return static_cast<act_t>(r >= up ? r - up : r);
    };
    if (L0 && VAL) {
        const act_t* const src[2] = {Dj, Vb};
        const int64_t ld[2] = {N, Nc};
        col_walk_n<kChunk, 2>(src, ld, n, [&](int c, const uint32_t (&x)[2]) {
            NV[static_cast<int64_t>(c) * Nn] = gate_digit(sve, svg, gv.ypr, x[0], x[1]);
            NI[static_cast<int64_t>(c) * Nn] = static_cast<act_t>(sc.next(m));
        });
    } else if (L0) {
        for (int c = 0; c < n; ++c) NI[static_cast<int64_t>(c) * Nn] = static_cast<act_t>(sc.next(m));
    } else {
        const act_t* Ej = ed.p[j] + gb * N + e;
        const act_t* Ib = i.p[j] + gb * Nc + sb;  // unread labels of a public b: inside the buffer, masked below
        if (VAL) {
            const act_t* const src[4] = {Dj, Vb, Ej, Ib};
            const int64_t ld[4] = {N, Nc, N, Nc};
            col_walk_n<kChunk, 4>(src, ld, n, [&](int c, const uint32_t (&x)[4]) {
                NV[static_cast<int64_t>(c) * Nn] = gate_digit(sve, svg, gv.ypr, x[0], x[1]);
                NI[static_cast<int64_t>(c) * Nn] = gate_digit(sie, sig, gi.ypr, x[2], ib_secret ? x[3] : 0u);
            });
        } else {
            const act_t* const src[2] = {Ej, Ib};
            const int64_t ld[2] = {N, Nc};
            col_walk_n<kChunk, 2>(src, ld, n, [&](int c, const uint32_t (&x)[2]) {
                NI[static_cast<int64_t>(c) * Nn] = gate_digit(sie, sig, gi.ypr, x[0], ib_secret ? x[1] : 0u);
            });
        }
    }
    // the carried slot cnt - 1 -> slot ops of the next level (cnt odd, never at the root), by the lanes of q = 0
    if (VAL && (a.cnt & 1) && e < P) {
        const int64_t from = static_cast<int64_t>(a.cnt - 1) * P + e, to = static_cast<int64_t>(a.ops) * P + e;
        const act_t* Vs = v.p[j] + gb * Nc + from;
        act_t* Vd = nv.p[j] + gb * Nn + to;
        for (int c = 0; c < n; ++c) Vd[static_cast<int64_t>(c) * Nn] = Vs[static_cast<int64_t>(c) * Nc];
        if (!L0 && a.carry_idx) {
            const act_t* Is = i.p[j] + gb * Nc + from;
            act_t* Id = ni.p[j] + gb * Nn + to;
            for (int c = 0; c < n; ++c) Id[static_cast<int64_t>(c) * Nn] = Is[static_cast<int64_t>(c) * Nc];
        }
    }
}

// ---------------------------------------------------------------------------
// Rescale step 1+2 for one factor: hash the factor residue (optionally after
// the upshift). grid (ceil(N/256), 1, B)
__global__ __launch_bounds__(kAesBlock, kAesMinBlocks) void k_rescale_hash(Act x, int fi, int s, const int16_t* up, int up_stride,
                                                      int add_up, int64_t N, u128* h0, uint16_t* col0,
                                                      const ModC* mc, const uint32_t* te0, const uint32_t* rk,
                                                      int hard) {
    AES_PROLOGUE(te0, rk);
    const int b = blockIdx.z;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const ModC m = mc[s];
    const act_t* L = x.p[fi] + static_cast<int64_t>(b) * m.n * N + e;
    const int16_t* U = up + static_cast<int64_t>(b) * up_stride;
    // compress of (L + up) mod s, streamed from the least significant component
    CompressFwd cf;
    cf.init();
    uint32_t c0 = 0;
    const int n = static_cast<int>(m.n);
    for (int i0 = 0; i0 < n; i0 += kChunk) {
        uint16_t lv[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u)
            if (i0 + u < n) lv[u] = static_cast<uint16_t>(L[(i0 + u) * N]);
#pragma unroll
        for (int u = 0; u < kChunk; ++u)
            if (i0 + u < n) {
                uint32_t d = lv[u];
                if (add_up) {
                    d += static_cast<uint16_t>(U[i0 + u]);
                    if (d >= static_cast<uint32_t>(s)) d -= s;
                }
                if (i0 + u == 0) c0 = d;
                cf.push(d, m);
            }
    }
    // hardened: the key itself (each active residue's update lane derives its own pad, k_rescale_update)
    h0[static_cast<int64_t>(b) * N + e] = hard ? cf.finish() : aes_encrypt(aes, cf.finish());
    col0[static_cast<int64_t>(b) * N + e] = static_cast<uint16_t>(c0);
    }
}


// grid (ceil(N/256), k, B)
__global__ __launch_bounds__(256) void k_rescale_update(RescaleArgs a, Act x, const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    act_t* L = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    const int16_t* U = a.up + static_cast<int64_t>(b) * a.lab_stride + a.lab_off[j];
    if (j == a.fi) {
        const int16_t* Zl = a.zero + static_cast<int64_t>(b) * a.lab_stride + a.lab_off[j];
        for (int i = 0; i < static_cast<int>(m.n); ++i) L[i * N] = Zl[i];
        return;
    }
    if (!a.active[j]) return;  // residue of an earlier factor (already zero)
    const int64_t be = static_cast<int64_t>(b) * N + e;
    const u128 mask = a.hard ? hard_pad(a.h0[be], a.gate0 ^ static_cast<uint64_t>(e), tw_sub(kTwTrans, a.factor), a.aidx[j])
                             : a.h0[be];
    const u128 P = a.trans[be * a.n_trans + a.off + static_cast<int64_t>(a.aidx[j]) * a.s + a.col0[be]] - mask;
    DigitStream s;
    s.init(P);
    const int32_t inv = a.inv[j];
    const int n = static_cast<int>(m.n);
    for (int i0 = 0; i0 < n; i0 += kChunk) {
        int16_t lv[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u)
            if (i0 + u < n) lv[u] = L[(i0 + u) * N];
#pragma unroll
        for (int u = 0; u < kChunk; ++u)
            if (i0 + u < n) {
                uint32_t v = static_cast<uint32_t>(lv[u]) + static_cast<uint32_t>(p) - s.next(m);  // [1, 2p)
                if (a.add_up) v += static_cast<uint32_t>(U[i0 + u]);
                L[(i0 + u) * N] = static_cast<act_t>(modq(v * static_cast<uint32_t>(inv), m));
            }
    }
}

// Downshift (and, for sign base extension, install the recovered mod-2 residue).
// grid (ceil(N/256), k, B)
__global__ __launch_bounds__(256) void k_rescale_post(Act x, CrtInfo crt, int64_t N, const u128* signP,
                                                      const int16_t* down, int lab_stride, const int* lab_off,
                                                      const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int p = crt.p[j];
    const ModC m = mc[p];
    act_t* L = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    const int16_t* D = down + static_cast<int64_t>(b) * lab_stride + lab_off[j];
    const int n = static_cast<int>(m.n);
    if (j == 0 && signP) {
        DigitStream s;
        s.init(signP[static_cast<int64_t>(b) * N + e]);
        for (int i = 0; i < n; ++i) {
            int32_t v = static_cast<int32_t>(s.next(m)) - D[i];
            L[i * N] = static_cast<act_t>(v < 0 ? v + p : v);
        }
        return;
    }
    for (int i0 = 0; i0 < n; i0 += kChunk) {
        int16_t lv[kChunk], dv[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u)
            if (i0 + u < n) {
                lv[u] = L[(i0 + u) * N];
                dv[u] = D[i0 + u];
            }
#pragma unroll
        for (int u = 0; u < kChunk; ++u)
            if (i0 + u < n) {
                const int32_t v = lv[u] - dv[u];
                L[(i0 + u) * N] = static_cast<act_t>(v < 0 ? v + p : v);
            }
    }
}


// ---------------------------------------------------------------------------
// Legacy (DASH) rescale, fused per iteration:
//   hash   : residue-0 key from the previous iteration's sign payload bits
//            (mod-2 labels: +/- is XOR, so no decompress at all)
//   update : L_j = (L_j + delta_j - proj(L_0)) * 2^-1 streamed digit by digit,
//            compressed on the fly and hashed -> approx projections of the
//            next sign gadget (phase A) in the same pass.
// The downshift of iteration i and the upshift of i+1 collapse into one
// delta = up - down; only the last iteration writes a downshifted result.
__global__ __launch_bounds__(kAesBlock, kAesMinBlocks) void k_rescale_hash_sign(const u128* signP, const u128* du, int64_t N, u128* h0,
                                                           uint16_t* col0, const uint32_t* te0, const uint32_t* rk) {
    AES_PROLOGUE(te0, rk);
    const int b = blockIdx.z;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const u128 C = signP[static_cast<int64_t>(b) * N + e] ^ du[b];
    h0[static_cast<int64_t>(b) * N + e] = aes_encrypt(aes, C);
    col0[static_cast<int64_t>(b) * N + e] = static_cast<uint16_t>(static_cast<uint32_t>(C) & 1u);
    }
}

// grid (x, k, B). Each component chunk is one dependent HBM round trip (the
// in-place stores keep the next chunk's loads behind them), so the chunk size
// sets the round trips per label; the t approx entries stay live across the
// loop, so larger chunks need the 128-VGPR budget (free here: the 64 KiB AES
// image already limits a CU to 16 waves).
#ifndef DASH_UA_CHUNK
#define DASH_UA_CHUNK 4
#endif
// the mixed-radix chain keeps K-1 digit streams live: at 6 waves/SIMD (80 VGPRs) it spills 240 B per
// lane; 4 waves/SIMD with 128 VGPRs measured faster (6.36 vs 7.04 ms per 24-GC MiniONN step)
constexpr int kChunkUA = DASH_UA_CHUNK;
// CH: components per dependent round trip. Latency-bound launches (batch 1, few waves per SIMD) take 16 (the
// label's n / 4 round trips, 32 for the 128 components of p = 2, were the floor of a small launch)
template <int TM, int CH>
__global__ __launch_bounds__(kAesBlock, DASH_UA_MINBLOCKS) void k_rescale_update_approx(RescaleArgs r, SignArgs a, Act x, const int16_t* delta,
                                                               const u128* zh, const ModC* mc, const uint32_t* te0,
                                                               const uint32_t* rk) {
    AES_PROLOGUE(te0, rk);
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = r.N;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int p = r.crt.p[j];
    const ModC m = mc[p];
    const int64_t be = static_cast<int64_t>(b) * N + e;
    const u128* TA = a.approx + be * a.n_approx + static_cast<int64_t>(a.t) * a.crt.prefix[j];
    u128 H;
    uint32_t col;
    u128 ent[TM];
    if (j == r.fi) {
        // factor residue is the zero label: constant key per GC
        H = zh[static_cast<int64_t>(b) * a.zc_stride + p];
        col = a.zcol[static_cast<int64_t>(b) * a.zc_stride + p];
#pragma unroll
        for (int d = 0; d < TM; ++d)
            if (d < a.t) ent[d] = TA[col * a.t + d];
    } else {
        const u128 Tt = r.trans[be * r.n_trans + static_cast<int64_t>(r.aidx[j]) * r.s + r.col0[be]];
        const u128 P = Tt - r.h0[be];
        act_t* L = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
        const int16_t* Dl = delta + static_cast<int64_t>(b) * r.lab_stride + r.lab_off[j];
        DigitStream s;
        s.init(P);
        CompressFwd cf;
        cf.init();
        const int32_t inv = r.inv[j];
        col = 0;
        const int n = static_cast<int>(m.n);
        for (int i0 = 0; i0 < n; i0 += CH) {
            int16_t lv[CH], dv[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if (i0 + u < n) {
                    lv[u] = L[(i0 + u) * N];
                    dv[u] = Dl[i0 + u];
                }
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if (i0 + u < n) {
                    // lv, dv, digit in [0, p): the sum is in [1, 3p), (sum * inv) mod p in one reduction
                    const uint32_t v = modq((static_cast<uint32_t>(lv[u]) + static_cast<uint32_t>(dv[u]) +
                                             static_cast<uint32_t>(p) - s.next(m)) * static_cast<uint32_t>(inv), m);
                    L[(i0 + u) * N] = static_cast<act_t>(v);
                    cf.push(v, m);
                    if (i0 + u == 0) {
                        col = static_cast<uint32_t>(v);
#pragma unroll
                        for (int d = 0; d < TM; ++d)
                            if (d < a.t) ent[d] = TA[col * a.t + d];
                    }
                }
        }
        H = aes_encrypt(aes, cf.finish());
    }
#pragma unroll
    for (int d = 0; d < TM; ++d)
        if (d < a.t) ent[d] -= H;
    approx_casts_out<TM>(aes, a, mc, j, b, e, ent, TA, col, H);
    }
}



void launch_rescale_hash_sign(const u128* signP, const u128* du, int64_t N, int B, u128* h0, uint16_t* col0,
                              const AesGlobals& g, hipStream_t st) {
    AES_LAUNCH_GGL(k_rescale_hash_sign, N, 1, B, kAesLds, st, signP, du, N, h0, col0, g.te0, g.rk);
}
void launch_rescale_update_approx(const RescaleArgs& r, const SignArgs& a, const Act& x, const int16_t* delta,
                                  const u128* zh, int B, const ModC* mc, const AesGlobals& g, hipStream_t st) {
    // DASH_UA_SMALL=0 keeps the throughput chunk on small launches (A/B)
    static const bool small_on = [] {
        const char* e = std::getenv("DASH_UA_SMALL");
        return !(e && e[0] == '0');
    }();
    // at most two waves per SIMD: the lanes are serial chains of round trips
    const bool small = small_on && r.N * r.crt.k * B <= static_cast<int64_t>(2 * 4 * 64) * num_cus();
    const LaunchDims d = aes_dims(small ? "update_approx.small" : "update_approx.large", r.N, r.crt.k, B);
    if (a.t <= 5 && small)
        hipLaunchKernelGGL((k_rescale_update_approx<5, 16>), d.grid, d.block, kAesLds, st, r, a, x, delta, zh, mc,
                           g.te0, g.rk);
    else if (a.t <= 5)
        hipLaunchKernelGGL((k_rescale_update_approx<5, kChunkUA>), d.grid, d.block, kAesLds, st, r, a, x, delta, zh,
                           mc, g.te0, g.rk);
    else if (small)
        hipLaunchKernelGGL((k_rescale_update_approx<8, 16>), d.grid, d.block, kAesLds, st, r, a, x, delta, zh, mc,
                           g.te0, g.rk);
    else
        hipLaunchKernelGGL((k_rescale_update_approx<8, kChunkUA>), d.grid, d.block, kAesLds, st, r, a, x, delta, zh,
                           mc, g.te0, g.rk);
}



// Output: Y_0 = pf_0 (mod 2), Y_j = S^-1 L_j + pf_j (mod p_j), in place. grid (ceil(N/256), k, B)
__global__ __launch_bounds__(256) void k_rescale_mrs_out(MrsArgs a, Act x, const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int k = a.crt.k;
    const ModC m = mc[a.crt.p[j]];
    const int n = static_cast<int>(m.n);
    act_t* L = x.p[j] + static_cast<int64_t>(b) * n * N + e;
    DigitStream s;
    s.init(a.pf[(static_cast<int64_t>(b) * k + j) * N + e]);
    if (j == 0) {
        for (int c = 0; c < n; ++c) L[static_cast<int64_t>(c) * N] = static_cast<act_t>(s.next(m));
        return;
    }
    const uint32_t inv = static_cast<uint32_t>(a.sinv[j]);
    // 16-digit groups: this kernel runs one short serial walk per lane (batch-1 launches are latency-bound), so
    // fewer, deeper round trips
    col_walk<2 * kChunk>(L, L, N, n, [&](int, uint32_t l) { return modq(l * inv + s.next(m), m); });  // < p^2 + p
}

// Joint rescale + ReLU (MODE 2): the output kernel also produces the next ReLU's garbler half-gate keys
// hx[b][j][e] = H(compress(Y_j)), colx = color (k_label_hash's job) from the components it writes, so the
// rescaled labels are not read back. Residue 0's output is the decompressed payload, its compress the payload.
__global__ __launch_bounds__(kAesBlock, kAesMinBlocks) void k_rescale_mrs_out_hash(MrsArgs a, Act x, const ModC* mc,
                                                                                  const uint32_t* te0,
                                                                                  const uint32_t* rk) {
    (void)te0;
    (void)rk;
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k;
    const ModC m = mc[a.crt.p[j]];
    const int n = static_cast<int>(m.n);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        act_t* L = x.p[j] + static_cast<int64_t>(b) * n * N + e;
        const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + e;
        const u128 P = a.pf[bke];
        DigitStream s;
        s.init(P);
        if (j == 0) {
            uint32_t c0 = 0;
            for (int c = 0; c < n; ++c) {
                const uint32_t v = s.next(m);
                if (c == 0) c0 = v;
                L[static_cast<int64_t>(c) * N] = static_cast<act_t>(v);
            }
            a.colx[bke] = static_cast<uint16_t>(c0);
            a.hx[bke] = hard_pad(P, a.rgate0 ^ static_cast<uint64_t>(e), tw_sub(kTwMmg, 0), 0);  // next ReLU g row
            continue;
        }
        const uint32_t inv = static_cast<uint32_t>(a.sinv[j]);
        CompressFwd cf;
        cf.init();
        uint32_t c0 = 0;
        col_walk<kChunk>(L, L, N, n, [&](int c, uint32_t l) {
            const uint32_t v = modq(l * inv + s.next(m), m);  // < p^2 + p
            if (c == 0) c0 = v;
            cf.push(v, m);
            return v;
        });
        a.colx[bke] = static_cast<uint16_t>(c0);
        a.hx[bke] = hard_pad(cf.finish(), a.rgate0 ^ static_cast<uint64_t>(e), tw_sub(kTwMmg, j), 0);
    }
}

// k_rescale_mrs_out_hash with the label staged in LDS (stage_ok): a block = (512-element tile, residue j,
// GC b) walks the label kOhCap components per pass: stage the rows, each lane rewrites its column in place,
// store the rows back (residue 0 only writes the decompressed payload).
constexpr int kOhBS = 512;
constexpr int kOhCap = 40;  // 20 KiB image beside the 32 KiB AES image: three blocks per CU
__global__ __launch_bounds__(kOhBS, kAesMinBlocks) void k_rescale_mrs_out_hash_s(MrsArgs a, Act x, const ModC* mc,
                                                                               const uint32_t* te0, const uint32_t* rk) {
    (void)te0;
    (void)rk;
    __shared__ __attribute__((aligned(16))) uint8_t stg[kOhCap * kOhBS];
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k;
    const ModC m = mc[a.crt.p[j]];
    const int n = static_cast<int>(m.n);
    const int tid = static_cast<int>(threadIdx.x);
    act_t* L = x.p[j] + static_cast<int64_t>(b) * n * N;
    const uint32_t inv = static_cast<uint32_t>(a.sinv[j]);
    for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kOhBS; e0 < N; e0 += static_cast<int64_t>(gridDim.x) * kOhBS) {
        const bool valid = e0 + tid < N;
        const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + (valid ? e0 + tid : N - 1);
        const u128 P = a.pf[bke];
        DigitStream s;
        s.init(P);
        CompressFwd cf;
        cf.init();
        ChunkKey ck;  // chunk-major state (non-power-of-two moduli)
        ck.init(P);
        uint32_t c0 = 0;
        // passes of whole chunks of m.c digits for the chunk-major walk
        const int pass = m.bits ? kOhCap : kOhCap / static_cast<int>(m.c) * static_cast<int>(m.c);
        for (int q0 = 0; q0 < n; q0 += pass) {
            const int cnt = min(pass, n - q0);
            __syncthreads();  // the previous pass's stores have read the image
            if (j != 0) {
                lds_stage_rows<kOhBS, 2>(stg, L, N, e0, q0, cnt);
                __syncthreads();
            }
            if (m.bits && cnt * static_cast<int>(m.bits) <= 64) {
                // power-of-two modulus, the pass's digits in one 64-bit window (residue 0 of the DASH bases: 128
                // one-bit digits, 40 per pass): a shift-and per digit over a fully unrolled, compile-time loop
                // instead of a 128-bit stream shift and scalar loop bookkeeping per digit (24-GC step -1.8 %,
                // profiles/ab/README.md round 6)
                const uint64_t win = static_cast<uint64_t>(s.Q);
                const uint32_t b = m.bits, msk = m.q - 1;
#pragma unroll
                for (int c = 0; c < kOhCap; ++c) {
                    if (c < cnt) {
                        uint8_t& w = stg[c * kOhBS + tid];
                        const uint32_t d = static_cast<uint32_t>(win >> (c * b)) & msk;
                        const uint32_t v = j == 0 ? d : modq(static_cast<uint32_t>(w) * inv + d, m);
                        w = static_cast<uint8_t>(v);
                        if (j != 0) cf.push(v, m);
                    }
                }
                s.Q >>= cnt * b;
                if (q0 == 0) c0 = stg[tid];  // digit 0 of the output (this lane's own LDS byte)
            } else if (m.bits) {
                for (int c = 0; c < cnt; ++c) {
                    uint8_t& w = stg[c * kOhBS + tid];
                    const uint32_t v = j == 0 ? s.next(m) : modq(static_cast<uint32_t>(w) * inv + s.next(m), m);
                    if (q0 + c == 0) c0 = v;
                    w = static_cast<uint8_t>(v);
                    if (j != 0) cf.push(v, m);
                }
            } else {
                ck.walk<kOhBS>(stg + tid, cnt, inv, j == 0, m);
                if (q0 == 0) c0 = stg[tid];  // digit 0 of the output (this lane's own LDS byte)
            }
            __syncthreads();
            lds_store_rows<kOhBS>(L, stg, N, e0, q0, cnt);
        }
        const u128 H = hard_pad(j == 0 ? P : (m.bits ? cf.finish() : ck.C),
                                a.rgate0 ^ static_cast<uint64_t>(valid ? e0 + tid : N - 1), tw_sub(kTwMmg, j), 0);
        if (valid) {
            a.colx[bke] = static_cast<uint16_t>(c0);
            a.hx[bke] = H;
        }
    }
}

// Joint rescale + ReLU, both outputs in one pass per (element, residue): Y_j (the rescaled label, written in
// place), its hash -> the garbler half gate G = g[color(Y_j)] - H(Y_j) (gathered as soon as the first
// component is known), then relu_j = E + ypr * Y_j - G (k_relu_mult's arithmetic) streamed into y while Y_j
// is read back from the lines this lane just wrote. The sign's hash / color come from chain MODE 2.
#ifndef DASH_RRO_WAVES
#define DASH_RRO_WAVES 4  // k_rescale_relu_out register budget (waves per SIMD): 6 spilled 256 B per lane
#endif
__global__ __launch_bounds__(kAesBlock, DASH_RRO_WAVES) void k_rescale_relu_out(MrsArgs a, SignArgs sa, Act x, Act y,
                                                                              const u128* gtab, const u128* etab,
                                                                              const ModC* mc, const uint32_t* te0,
                                                                              const uint32_t* rk) {
    (void)te0;
    (void)rk;
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const uint32_t inv = static_cast<uint32_t>(a.sinv[j]);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t be = static_cast<int64_t>(b) * N + e;
        const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + e;
        act_t* L = x.p[j] + static_cast<int64_t>(b) * n * N + e;
        act_t* Y = y.p[j] + static_cast<int64_t>(b) * n * N + e;
        const ReluOps o = relu_ops(nullptr, a.ys, a.ny, a.cs, etab, b, j, k, N, e);
        const u128* grow = gtab + be * sa.crt.sum + sa.crt.prefix[j];
        const u128 P = a.pf[bke];
        DigitStream s;
        s.init(P);
        u128 key, Graw;
        if (j == 0) {
            // Y_0 = decompress(P), compress(Y_0) = P
            uint32_t c0 = 0;
            for (int c = 0; c < n; ++c) {
                const uint32_t v = s.next(m);
                if (c == 0) {
                    c0 = v;
                    Graw = grow[c0];
                }
                L[static_cast<int64_t>(c) * N] = static_cast<act_t>(v);
            }
            key = P;
        } else {
            CompressFwd cf;
            cf.init();
            col_walk<kChunk>(L, L, N, n, [&](int c, uint32_t l) {
                const uint32_t v = modq(l * inv + s.next(m), m);  // < p^2 + p
                if (c == 0) Graw = grow[v];
                cf.push(v, m);
                return v;
            });
            key = cf.finish();
        }
        const u128 G = Graw - hard_pad(key, a.rgate0 ^ static_cast<uint64_t>(e), tw_sub(kTwMmg, j), 0);
        const uint32_t ypr = mini_mult(o.mini, o.cS, o.HM, p, m);
        DigitStream sg, se;
        sg.init(G);
        se.init(o.Eraw - o.HS);
        // col_walk<kChunk>(L, Y, ...) written out: through the helper this second walk is allocated 74 registers
        // for the parent's 87 and the kernel's occupancy moves from 5 to 6 waves per SIMD
        // (profiles/ab/gadget_walks/README.md)
        uint16_t cur[kChunk], nxt[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u)
            if (u < n) cur[u] = L[static_cast<int64_t>(u) * N];
        for (int i0 = 0; i0 < n; i0 += kChunk) {
#pragma unroll
            for (int u = 0; u < kChunk; ++u)
                if (i0 + kChunk + u < n) nxt[u] = L[static_cast<int64_t>(i0 + kChunk + u) * N];
#pragma unroll
            for (int u = 0; u < kChunk; ++u)
                if (i0 + u < n) {
                    const uint32_t g = sg.next(m);
                    const uint32_t ev = se.next(m);
                    Y[static_cast<int64_t>(i0 + u) * N] = static_cast<act_t>(mult_digit(ev, ypr, cur[u], p, g, m));
                }
#pragma unroll
            for (int u = 0; u < kChunk; ++u) cur[u] = nxt[u];
        }
    }
}

// k_rescale_relu_out with the label staged in LDS (stage_ok, small batches): a block = (256-element tile,
// residue j, GC b) brings x_j's rows in once as 16-byte loads, each lane rescales its column in place and
// hashes it (the rescaled label stays in LDS: nothing reads it after a deferred rescale), then rewrites its
// column into the ReLU output, stored as rows. The per-lane form streams the label twice with one byte per
// lane per load, n / kChunk dependent round trips per pass. Measured at batch 1 (MiniONN, round 4, when it
// still stored the rescaled rows): 90 us per op vs 76 for the per-lane form and ~50 + ~50 for the staged
// output-hash and ReLU-multiply kernels. Batches of at most 2 GCs take it; larger ones k_rescale_relu_out_t.
constexpr int kRroBS = 256;
__global__ __launch_bounds__(kRroBS) void k_rescale_relu_out_s(MrsArgs a, SignArgs sa, Act x, Act y, const u128* gtab,
                                                                const u128* etab, const ModC* mc, const uint32_t* te0,
                                                                const uint32_t* rk) {
    (void)te0;
    (void)rk;
    __shared__ __attribute__((aligned(16))) uint8_t stg[128 * kRroBS];
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const int tid = static_cast<int>(threadIdx.x);
    const uint32_t inv = static_cast<uint32_t>(a.sinv[j]);
    act_t* L = x.p[j] + static_cast<int64_t>(b) * n * N;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * n * N;
    for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRroBS; e0 < N; e0 += static_cast<int64_t>(gridDim.x) * kRroBS) {
        const int64_t e = min(e0 + tid, N - 1);  // spare lanes shadow a real element; the row stores skip them
        const int64_t be = static_cast<int64_t>(b) * N + e;
        const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + e;
        const ReluOps o = relu_ops(nullptr, a.ys, a.ny, a.cs, etab, b, j, k, N, e);
        const u128* grow = gtab + be * sa.crt.sum + sa.crt.prefix[j];
        const u128 P = a.pf[bke];
        __syncthreads();  // the previous tile's row stores have read the image
        if (j != 0) lds_stage_rows<kRroBS, 4>(stg, L, N, e0, 0, n);
        __syncthreads();
        uint8_t* col = stg + tid;
        DigitStream s;
        s.init(P);
        CompressFwd cf;
        cf.init();
        u128 Graw = 0;
        constexpr int kRroG = 8;  // digits per grouped LDS read (lds_group_walk)
        // p = 2: Y_0's digits are the bits of P. Its 128 components are the longest label, so the residue-0 blocks
        // were the launch's tail when each digit took a 128-bit stream shift. (The walks below get a row count of
        // 0 instead of sitting in an else: as an if / else the kernel takes 115 registers for 85.)
        const bool bits0 = j == 0 && m.bits == 1;
        if (bits0) {
            Graw = grow[static_cast<uint32_t>(P) & 1u];
            lds_bit_rows<kRroBS>(col, n, P, [](uint32_t bit, uint32_t) { return bit; });
        }
        lds_group_walk<kRroBS, kRroG>(col, bits0 ? 0 : n, j != 0, [&](int c, uint32_t l) {
            const uint32_t v = j == 0 ? s.next(m) : modq(l * inv + s.next(m), m);
            if (c == 0) Graw = grow[v];
            if (j != 0) cf.push(v, m);
            return v;
        });
        // Y_j stays in LDS: the planner fuses only where nothing reads the rescaled label again (runtime.hip defer)
        const u128 key = j == 0 ? P : cf.finish();
        const u128 G = Graw - hard_pad(key, a.rgate0 ^ static_cast<uint64_t>(e), tw_sub(kTwMmg, j), 0);
        const u128 E = o.Eraw - o.HS;
        const uint32_t ypr = mini_mult(o.mini, o.cS, o.HM, p, m);
        // each lane rereads only its own column of Y_j: no barrier between the passes
        DigitStream sg, se;
        sg.init(G);
        se.init(E);
        if (m.bits == 1) lds_bit_rows<kRroBS>(col, n, G ^ E, [=](uint32_t bit, uint32_t yv) { return bit ^ (yv & ypr); });
        lds_group_walk<kRroBS, kRroG>(col, m.bits == 1 ? 0 : n, true, [&](int, uint32_t yv) {
            const uint32_t g = sg.next(m);
            return mult_digit(se.next(m), ypr, yv, p, g, m);
        });
        __syncthreads();
        lds_store_rows<kRroBS>(Y, stg, N, e0, 0, n);
    }
}

// Throughput form of the joint output (batch >= 3, stage_ok): a block = (256-element tile, residue j, GC b).
// The rescaled label Y_j lives only in LDS: nothing is stored to x, and no hx / colx round trip (the two-kernel
// path writes and reads back n_j + 18 bytes per element and residue). Odd residues stage L_j once, rewrite it to
// Y_j with the chunk-major walk of k_rescale_mrs_out_hash_s (key summed per chunk), hash once, rewrite it to
// relu_j with the chunk-major walk of k_relu_mult_s and store the rows to y. Residue 0 (p = 2) needs no input
// rows: Y_0 is the bits of the payload P and relu_0 = (G ^ E) ^ (P & -ypr) on 128-bit registers; LDS only
// transposes the result bits into byte rows, kRrtCap rows per window. The image is kRrtCap rows (20 KiB); bases
// with a longer odd residue, or whose residue 0 is not p = 2, take k_rescale_relu_out_s (rrt_fits).
constexpr int kRrtBS = 256;
constexpr int kRrtCap = 80;
static inline bool rrt_fits(const MrsArgs& a) {
    bool fits = a.crt.p[0] == 2 && a.crt.n[0] <= 128;
    for (int j = 1; j < a.crt.k; ++j) fits = fits && (a.crt.p[j] & (a.crt.p[j] - 1)) != 0 && a.crt.n[j] <= kRrtCap;
    return fits;
}
// lds_stage_rows<kRrtBS, 4> with the four units in named registers: the helper's uint4 v[4], filled under a
// condition, stays an 80-byte stack object in this kernel (scratch)
__device__ __forceinline__ void rrt_stage_rows(uint8_t* S, const act_t* L, int64_t N, int64_t e0, int cnt) {
    constexpr int W = kRrtBS / 16;
    const int units = cnt * W;
    auto ld = [=](int xu) {
        const int64_t e = e0 + 16 * (xu % W);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (xu < units && e < N) v = *reinterpret_cast<const uint4*>(L + static_cast<int64_t>(xu / W) * N + e);
        return v;
    };
    auto st = [=](int xu, uint4 v) {
        if (xu < units) *reinterpret_cast<uint4*>(S + (xu / W) * kRrtBS + 16 * (xu % W)) = v;
    };
    for (int x0 = threadIdx.x; x0 < units; x0 += 4 * kRrtBS) {
        const uint4 v0 = ld(x0), v1 = ld(x0 + kRrtBS), v2 = ld(x0 + 2 * kRrtBS), v3 = ld(x0 + 3 * kRrtBS);
        st(x0, v0);
        st(x0 + kRrtBS, v1);
        st(x0 + 2 * kRrtBS, v2);
        st(x0 + 3 * kRrtBS, v3);
    }
}
// The kernel's body. LEAKY (k_rescale_leaky_out_t): pass 2 and residue 0 take the leaky epilogue b Y_j + c relu_j
// (gadgets.h LeakyPlan); the ReLU instantiation never reads lk.
template <bool LEAKY>
__device__ __forceinline__ void rescale_relu_out_t_body(uint8_t* stg, const MrsArgs& a, const SignArgs& sa,
                                                        const LeakyTab& lk, const Act& x, const Act& y,
                                                        const u128* gtab, const u128* etab, const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const int tid = static_cast<int>(threadIdx.x);
    const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRrtBS;
    const int64_t e = min(e0 + tid, N - 1);  // spare lanes shadow a real element; the row stores skip them
    const int64_t be = static_cast<int64_t>(b) * N + e;
    const act_t* L = x.p[j] + static_cast<int64_t>(b) * n * N;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * n * N;
    // the per-element gathers first: in flight while the rows are staged
    const u128 P = a.pf[(static_cast<int64_t>(b) * k + j) * N + e];
    const ReluOps o = relu_ops(nullptr, a.ys, a.ny, a.cs, etab, b, j, k, N, e);
    const u128* grow = gtab + be * sa.crt.sum + sa.crt.prefix[j];
    const uint64_t gate = a.rgate0 ^ static_cast<uint64_t>(e);
    uint8_t* col = stg + tid;
    if (j == 0) {
        const u128 Graw = grow[static_cast<uint32_t>(P) & 1u];
        const u128 G = Graw - hard_pad(P, gate, tw_sub(kTwMmg, 0), 0);  // compress(Y_0) = P
        const u128 E = o.Eraw - o.HS;
        const uint32_t t16 = static_cast<uint32_t>(o.mini >> (16 * o.cS)), hm = static_cast<uint32_t>(o.HM);
        // (e + ypr y + 2 - g) mod 2 = e ^ g ^ (ypr & y) with ypr = (t16 - hm) mod 2
        u128 R = (G ^ E) ^ (((t16 ^ hm) & 1u) ? P : static_cast<u128>(0));
        if (LEAKY) {  // (b & Y_0) ^ (c & relu_0) on the 128-bit words
            const LeakyLane ll = leaky_lane(lk, e, 0, k);
            R = (ll.fb ? P : static_cast<u128>(0)) ^ (ll.fc ? R : static_cast<u128>(0));
        }
        for (int q0 = 0; q0 < n; q0 += kRrtCap) {
            const int cnt = min(kRrtCap, n - q0);
            if (q0) __syncthreads();  // the previous window's row stores have read the image
            // lds_bit_rows written out (over kRrtCap rows): through the helper the residue-0 blocks, the longest
            // label of the headline's kernel, gain 68 instructions (profiles/ab/gadget_walks/README.md)
            const u128 Rw = R >> q0;
#pragma unroll
            for (int w = 0; w < (kRrtCap + 31) / 32; ++w) {
                const uint32_t rw = static_cast<uint32_t>(Rw >> (32 * w));
#pragma unroll 8
                for (int u = 0; u < 32; ++u) {
                    const int c = 32 * w + u;
                    if (c >= cnt) break;
                    stg[c * kRrtBS + tid] = static_cast<uint8_t>((rw >> u) & 1u);
                }
            }
            __syncthreads();
            lds_store_rows<kRrtBS>(Y, stg, N, e0, q0, cnt);
        }
        return;
    }
    const uint32_t inv = static_cast<uint32_t>(a.sinv[j]);
    rrt_stage_rows(stg, L, N, e0, n);
    __syncthreads();
    // digit 0 of Y_j ahead of the walk: the garbler half gate's row gather overlaps pass 1
    u128 Graw;
    {
        u128 t = P;
        uint32_t r = divmod128(t, m);
        const uint32_t pd0 = chunk_digit(r, m);
        Graw = grow[modq(static_cast<uint32_t>(stg[tid]) * inv + pd0, m)];
    }
    // pass 1: Y_j = S^-1 L_j + digits(P) in place, key = compress(Y_j) summed per chunk. The residue is
    // block-uniform: with a.cmod the odd primes up to kModKMax take the constant-modulus walks (one scalar branch
    // per pass), every other modulus the run-time forms
    u128 key = 0;
    const bool kform = a.cmod && modk_dispatch(static_cast<uint32_t>(p), [&](auto mk) __attribute__((always_inline)) {
        key = rescale_walk_k<decltype(mk), kRrtBS>(col, P, inv);
    });
    if (!kform) {
        ChunkKey ck;
        ck.init(P);
        ck.walk<kRrtBS>(col, n, inv, false, m);
        key = ck.C;
    }
    const u128 G = Graw - hard_pad(key, gate, tw_sub(kTwMmg, j), 0);
    // pass 2: relu_j = E + ypr Y_j - G in place
    const u128 E = o.Eraw - o.HS;
    const uint32_t ypr = mini_mult(o.mini, o.cS, o.HM, p, m);
    if (kform) {
        modk_dispatch(static_cast<uint32_t>(p), [&](auto mk) __attribute__((always_inline)) {
            if constexpr (LEAKY) lds_mult_chunks_k<decltype(mk), kRrtBS, false, true>(col, G, E, 0, ypr, leaky_lane(lk, e, j, k));
            else lds_mult_chunks_k<decltype(mk), kRrtBS, false>(col, G, E, 0, ypr);
        });
    } else if (LEAKY) {
        lds_mult_chunks<kRrtBS, false, true>(col, n, G, E, 0, ypr, p, m, leaky_lane(lk, e, j, k));
    } else {
        lds_mult_chunks<kRrtBS, false>(col, n, G, E, 0, ypr, p, m);
    }
    __syncthreads();
    lds_store_rows<kRrtBS>(Y, stg, N, e0, 0, n);
}
__global__ __launch_bounds__(kRrtBS) void k_rescale_relu_out_t(MrsArgs a, SignArgs sa, Act x, Act y, const u128* gtab,
                                                                const u128* etab, const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[kRrtCap * kRrtBS];
    rescale_relu_out_t_body<false>(stg, a, sa, LeakyTab{nullptr, 1u}, x, y, gtab, etab, mc);
}
// k_rescale_relu_out_t for a joint LeakyRelu: the same block, image and passes with the leaky epilogue
__global__ __launch_bounds__(kRrtBS) void k_rescale_leaky_out_t(MrsArgs a, SignArgs sa, LeakyTab lk, Act x, Act y,
                                                                 const u128* gtab, const u128* etab, const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[kRrtCap * kRrtBS];
    rescale_relu_out_t_body<true>(stg, a, sa, lk, x, y, gtab, etab, mc);
}

// k_rescale_relu_out_t for a joint Clip (gadgets.h ClipPlan, joint variant): the same block, image and two
// passes, with the clip multiply's rows instead of the ReLU's. The two sign labels come from the rescale chain
// (mode 2, ca.klo) and the Clip's upper sign chain (mode 1, ca.khi), which both ran on the rescale's input; the
// lane derives the pads of u and of s_hi (clip_keyed) while the rows are staged. Pass 2 adds the cap stream;
// residue 0 is (G ^ E ^ C) ^ (ypr ? P : 0) on 128-bit registers. The rescaled label is never written.
__global__ __launch_bounds__(kRrtBS, 5) void k_rescale_clip_out_t(MrsArgs a, ClipArgs ca, Act x, Act y, const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[kRrtCap * kRrtBS];
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const int tid = static_cast<int>(threadIdx.x);
    const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRrtBS;
    const int64_t e = min(e0 + tid, N - 1);  // spare lanes shadow a real element; the row stores skip them
    const int64_t be = static_cast<int64_t>(b) * N + e;
    const act_t* L = x.p[j] + static_cast<int64_t>(b) * n * N;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * n * N;
    // the per-element gathers first: in flight while the rows are staged
    const u128 P = a.pf[(static_cast<int64_t>(b) * k + j) * N + e];
    const u128* grow = ca.gtab + be * ca.crt.sum + ca.crt.prefix[j];
    const uint64_t gate = ca.mgate0 ^ static_cast<uint64_t>(e);
    uint8_t* col = stg + tid;
    if (j == 0) {
        const u128 Graw = grow[static_cast<uint32_t>(P) & 1u];
        const ClipLane c = clip_keyed(ca, j, b, e, p, m);
        const u128 G = Graw - hard_pad(P, gate, tw_sub(kTwMmg, 0), 0);  // compress(Y_0) = P
        // (e + c + ypr y + 2 - g) mod 2 = e ^ c ^ g ^ (ypr & y)
        const u128 R = (G ^ c.E ^ c.C) ^ ((c.ypr & 1u) ? P : static_cast<u128>(0));
        for (int q0 = 0; q0 < n; q0 += kRrtCap) {
            const int cnt = min(kRrtCap, n - q0);
            if (q0) __syncthreads();  // the previous window's row stores have read the image
            const u128 Rw = R >> q0;
#pragma unroll
            for (int w = 0; w < (kRrtCap + 31) / 32; ++w) {
                const uint32_t rw = static_cast<uint32_t>(Rw >> (32 * w));
#pragma unroll 8
                for (int u = 0; u < 32; ++u) {
                    const int cc = 32 * w + u;
                    if (cc >= cnt) break;
                    stg[cc * kRrtBS + tid] = static_cast<uint8_t>((rw >> u) & 1u);
                }
            }
            __syncthreads();
            lds_store_rows<kRrtBS>(Y, stg, N, e0, q0, cnt);
        }
        return;
    }
    const uint32_t inv = static_cast<uint32_t>(a.sinv[j]);
    rrt_stage_rows(stg, L, N, e0, n);
    __syncthreads();
    // digit 0 of Y_j ahead of the walk: the garbler half gate's row gather overlaps the pads and pass 1
    u128 Graw;
    {
        u128 t = P;
        uint32_t r = divmod128(t, m);
        const uint32_t pd0 = chunk_digit(r, m);
        Graw = grow[modq(static_cast<uint32_t>(stg[tid]) * inv + pd0, m)];
    }
    const ClipLane c = clip_keyed(ca, j, b, e, p, m);
    // pass 1: Y_j = S^-1 L_j + digits(P) in place, key = compress(Y_j) summed per chunk
    // (constant-modulus walks as in rescale_relu_out_t_body)
    u128 key = 0;
    const bool kform = a.cmod && modk_dispatch(static_cast<uint32_t>(p), [&](auto mk) __attribute__((always_inline)) {
        key = rescale_walk_k<decltype(mk), kRrtBS>(col, P, inv);
    });
    if (!kform) {
        ChunkKey ck;
        ck.init(P);
        ck.walk<kRrtBS>(col, n, inv, false, m);
        key = ck.C;
    }
    const u128 G = Graw - hard_pad(key, gate, tw_sub(kTwMmg, j), 0);
    // pass 2: clip_j = E + C + ypr Y_j - G in place
    if (kform)
        modk_dispatch(static_cast<uint32_t>(p), [&](auto mk) __attribute__((always_inline)) {
            lds_mult_chunks_k<decltype(mk), kRrtBS, true>(col, G, c.E, c.C, c.ypr);
        });
    else
        lds_mult_chunks<kRrtBS, true>(col, n, G, c.E, c.C, c.ypr, p, m);
    __syncthreads();
    lds_store_rows<kRrtBS>(Y, stg, N, e0, 0, n);
}

// Quad form of the joint output (latency-bound launches: batch 1, small layers). Four lanes per (element,
// residue): the label's base-q chunks are dealt over the quad (lane g takes chunks 4j + g, power-of-two moduli
// a quarter of the digits each), every lane runs the payload's chunk divisions and keeps its own chunk, the
// rescaled label's partial keys are summed over the quad. The per-lane forms walk all n digits of three streams
// serially on one lane (~50 us per launch whatever the layer size at batch 1, r05 timeline).
constexpr int kRroQE = 64;  // elements per block (256 threads)
// rows [0, n) of kRroQE elements from e0: 16-byte units when N % 16 == 0, bytes otherwise (tails, tiny layers)
__device__ __forceinline__ void quad_stage_rows(uint8_t* S, const act_t* L, int64_t N, int64_t e0, int n) {
    if (N % 16 == 0) {
        for (int xu = threadIdx.x; xu < n * (kRroQE / 16); xu += blockDim.x) {
            const int row = xu / (kRroQE / 16), part = xu % (kRroQE / 16);
            const int64_t ee = e0 + 16 * part;
            if (ee < N) *reinterpret_cast<uint4*>(S + row * kRroQE + 16 * part) =
                *reinterpret_cast<const uint4*>(L + static_cast<int64_t>(row) * N + ee);
        }
    } else {
        for (int xb = threadIdx.x; xb < n * kRroQE; xb += blockDim.x) {
            const int row = xb / kRroQE, c = xb % kRroQE;
            if (e0 + c < N) S[xb] = L[static_cast<int64_t>(row) * N + e0 + c];
        }
    }
}
__device__ __forceinline__ void quad_store_rows(act_t* L, const uint8_t* S, int64_t N, int64_t e0, int n) {
    if (N % 16 == 0) {
        for (int xu = threadIdx.x; xu < n * (kRroQE / 16); xu += blockDim.x) {
            const int row = xu / (kRroQE / 16), part = xu % (kRroQE / 16);
            const int64_t ee = e0 + 16 * part;
            if (ee < N) *reinterpret_cast<uint4*>(L + static_cast<int64_t>(row) * N + ee) =
                *reinterpret_cast<const uint4*>(S + row * kRroQE + 16 * part);
        }
    } else {
        for (int xb = threadIdx.x; xb < n * kRroQE; xb += blockDim.x) {
            const int row = xb / kRroQE, c = xb % kRroQE;
            if (e0 + c < N) L[static_cast<int64_t>(row) * N + e0 + c] = S[xb];
        }
    }
}
// the quad output forms where a lane-per-element launch would not fill the chip (latency-bound: batch 1, small
// layers); DASH_RRO_QUAD=0 keeps the lane-per-element forms, =2 takes the quad forms at every size (A/B)
static inline bool out_quad_fits(const MrsArgs& a, int B) {
    static const int mode = [] {
        const char* e = std::getenv("DASH_RRO_QUAD");
        return e ? std::atoi(e) : 1;
    }();
    bool fits = mode != 0 && (mode == 2 || (a.N + 255) / 256 * a.crt.k * B <= num_cus());
    for (int j = 0; j < a.crt.k; ++j) fits = fits && a.crt.n[j] <= 128;  // the LDS images hold 128 components
    return fits;
}
__global__ __launch_bounds__(256) void k_rescale_relu_out_q(MrsArgs a, SignArgs sa, Act x, Act y, const u128* gtab,
                                                           const u128* etab, const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t sL[128 * kRroQE];  // L_j -> Y_j in place
    __shared__ __attribute__((aligned(16))) uint8_t sO[128 * kRroQE];  // ReLU outputs
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const int tid = static_cast<int>(threadIdx.x);
    const int el = tid >> 2, g = tid & 3;
    const uint32_t inv = static_cast<uint32_t>(a.sinv[j]);
    act_t* L = x.p[j] + static_cast<int64_t>(b) * n * N;
    act_t* Yo = y.p[j] + static_cast<int64_t>(b) * n * N;
    for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRroQE; e0 < N; e0 += static_cast<int64_t>(gridDim.x) * kRroQE) {
        const int64_t e = min(e0 + el, N - 1);  // spare quads shadow a real element; the row stores skip them
        const int64_t be = static_cast<int64_t>(b) * N + e;
        const int64_t bke = (static_cast<int64_t>(b) * k + j) * N + e;
        const ReluOps o = relu_ops(nullptr, a.ys, a.ny, a.cs, etab, b, j, k, N, e);
        const u128* grow = gtab + be * sa.crt.sum + sa.crt.prefix[j];
        const u128 P = a.pf[bke];
        __syncthreads();  // the previous tile's row stores have read the images
        if (j != 0) quad_stage_rows(sL, L, N, e0, n);
        __syncthreads();
        // digit 0 first (every lane): the garbler half gate's row gather overlaps the walk
        u128 Graw;
        {
            uint32_t pd0;
            if (m.bits) {
                pd0 = static_cast<uint32_t>(P) & (m.q - 1);
            } else {
                u128 t = P;
                uint32_t r = divmod128(t, m);
                pd0 = chunk_digit(r, m);
            }
            const uint32_t v0 = j == 0 ? pd0 : modq(static_cast<uint32_t>(sL[el]) * inv + pd0, m);
            Graw = grow[v0];
        }
        // Y_j = S^-1 L_j + P (mod p), residue 0: Y_0 = decompress(P); the lane's digits and its partial key
        const u128 part = quad_rescale_walk<kRroQE, true>(sL + el, n, g, P, inv, j == 0, m);
        const u128 key = j == 0 ? P : quad_sum128(part);
        u128 G;
        if constexpr (kQCoop) {  // the quad runs the pad block together (every lane holds the same key)
            uint32_t w[4];
            hard_block_q(key, a.rgate0 ^ static_cast<uint64_t>(e), tw_sub(kTwMmg, j), 0u, g, w);
            G = Graw - quad_gather128(w[0]);
        } else {
            G = Graw - hard_pad(key, a.rgate0 ^ static_cast<uint64_t>(e), tw_sub(kTwMmg, j), 0);
        }
        // relu_j = E + ypr Y_j - G, the lane's own digits
        quad_mult_walk<kRroQE>(sL + el, sO + el, n, g, G, o.Eraw - o.HS, mini_mult(o.mini, o.cS, o.HM, p, m), p, m);
        __syncthreads();
        quad_store_rows(Yo, sO, N, e0, n);  // Y_j (sL) is not stored: nothing reads it again (runtime.hip defer)
    }
}

// Constant-modulus kernel forms (launch.h): the mode, initially DASH_CONST_MOD or kConstModDefault, and the counts
// of host-side launches that took a constant form (the launch log's lines are the same for both forms)
static std::atomic<int>& const_mod_state() {
    static std::atomic<int> mode{[] {
        const char* e = std::getenv("DASH_CONST_MOD");
        const int v = e ? std::atoi(e) : kConstModDefault;
        return v < 0 ? 0 : (v > 2 ? 2 : v);
    }()};
    return mode;
}
static std::atomic<long> g_cmod_chain{0}, g_cmod_out{0};
int const_mod_mode() { return const_mod_state().load(std::memory_order_relaxed); }
void set_const_mod(int mode) { const_mod_state().store(mode < 0 ? 0 : (mode > 2 ? 2 : mode), std::memory_order_relaxed); }
void const_mod_count(bool chain) { (chain ? g_cmod_chain : g_cmod_out).fetch_add(1, std::memory_order_relaxed); }
long const_mod_launches(bool chain) { return (chain ? g_cmod_chain : g_cmod_out).load(std::memory_order_relaxed); }

// The joint-fuse mode (launch.h): -1 auto, 0 off, 1 on; the DASH_JOINT_FUSE environment value is its initial state
static std::atomic<int>& joint_fuse_state() {
    static std::atomic<int> mode{[] {
        const char* e = std::getenv("DASH_JOINT_FUSE");
        const int v = e ? std::atoi(e) : -1;
        return v > 0 ? 1 : (v == 0 ? 0 : -1);
    }()};
    return mode;
}
int joint_fuse_mode() { return joint_fuse_state().load(std::memory_order_relaxed); }
void set_joint_fuse(int mode) { joint_fuse_state().store(mode > 0 ? 1 : (mode == 0 ? 0 : -1), std::memory_order_relaxed); }
// Threshold on batch * N for batches above 2: the smallest launch measured, 24 GCs x 576 elements, where the
// layer's rescale and ReLU ops (chain included) take 0.088 ms fused against 0.129 ms with the output-hash and
// ReLU-multiply kernels (every larger MiniONN layer wins too, profiles/ab/joint_fused/README.md). Nothing smaller was measured at batch >= 3, so nothing smaller fuses
// (tests/test_gpu_launch_forms.py pins the two-kernel path up to 3 x 2064 = 6192 elements).
constexpr int64_t kJointFuseMinElems = 24 * 576;
int64_t joint_fuse_min_elems() { return kJointFuseMinElems; }
bool joint_fuse_pick(int64_t N, int B) { return B <= 2 || (stage_ok(N, kRrtBS) && B * N >= kJointFuseMinElems); }
bool joint_fuse(int64_t N, int B) {
    const int mode = joint_fuse_mode();
    return mode >= 0 ? mode == 1 : joint_fuse_pick(N, B);
}

bool leaky_fuse(int64_t N, int B) {
    const int mode = joint_fuse_mode();
    return mode >= 0 ? mode == 1 : (B >= 3 && joint_fuse_pick(N, B));
}

void launch_rescale_relu_out(const MrsArgs& a, const SignArgs& sa, const Act& x, const Act& y, const u128* gtab,
                             const u128* etab, int B, const ModC* mc, const AesGlobals& g, hipStream_t st) {
    static const bool rro_stage = [] {  // DASH_RRO_STAGE=0: the per-lane form (A/B)
        const char* e = std::getenv("DASH_RRO_STAGE");
        return !(e && e[0] == '0');
    }();
    if (out_quad_fits(a, B)) {
        const dim3 gq(static_cast<unsigned>((a.N + kRroQE - 1) / kRroQE), a.crt.k, B);
        if (launch_log_on()) launch_log_add("relu_out.quad", gq, dim3(256));
        hipLaunchKernelGGL(k_rescale_relu_out_q, gq, dim3(256), 0, st, a, sa, x, y, gtab, etab, mc);
        return;
    }
    if (rro_stage && B >= 3 && stage_ok(a.N, kRrtBS) && rrt_fits(a)) {  // throughput batches (own log name)
        const dim3 gt(static_cast<unsigned>((a.N + kRrtBS - 1) / kRrtBS), a.crt.k, B);
        if (launch_log_on()) launch_log_add("relu_out.tput", gt, dim3(kRrtBS));
        MrsArgs ak = a;
        ak.cmod = const_mod_on() ? 1 : 0;
        if (ak.cmod) const_mod_count(false);
        hipLaunchKernelGGL(k_rescale_relu_out_t, gt, dim3(kRrtBS), 0, st, ak, sa, x, y, gtab, etab, mc);
        return;
    }
    if (rro_stage && stage_ok(a.N, kRroBS)) {
        const dim3 gs(static_cast<unsigned>((a.N + kRroBS - 1) / kRroBS), a.crt.k, B);
        if (launch_log_on()) launch_log_add("relu_out.staged", gs, dim3(kRroBS));
        hipLaunchKernelGGL(k_rescale_relu_out_s, gs, dim3(kRroBS), 0, st, a, sa, x, y, gtab, etab, mc, g.te0, g.rk);
        return;
    }
    const LaunchDims d = aes_dims("relu_out.lane", a.N, a.crt.k, B);
    hipLaunchKernelGGL(k_rescale_relu_out, d.grid, d.block, kAesLds, st, a, sa, x, y, gtab, etab, mc, g.te0, g.rk);
}

// The deferred outputs of a rescale with a joint LeakyRelu behind it. The throughput form where
// launch_rescale_relu_out takes its own (the same rule); the small-batch fused forms (quad, staged, lane) have
// no leaky counterpart: those launches run the rescale's output-hash kernel and the leaky multiply.
void launch_rescale_leaky_out(const MrsArgs& a, const SignArgs& sa, const LeakyTab& lk, const Act& x, const Act& y,
                              const u128* gtab, const u128* etab, int B, const ModC* mc, const AesGlobals& g,
                              hipStream_t st) {
    static const bool rro_stage = [] {  // DASH_RRO_STAGE=0, as launch_rescale_relu_out
        const char* e = std::getenv("DASH_RRO_STAGE");
        return !(e && e[0] == '0');
    }();
    if (!out_quad_fits(a, B) && rro_stage && B >= 3 && stage_ok(a.N, kRrtBS) && rrt_fits(a)) {
        const dim3 gt(static_cast<unsigned>((a.N + kRrtBS - 1) / kRrtBS), a.crt.k, B);
        if (launch_log_on()) launch_log_add("leaky_out.tput", gt, dim3(kRrtBS));
        MrsArgs ak = a;
        ak.cmod = const_mod_on() ? 1 : 0;
        if (ak.cmod) const_mod_count(false);
        hipLaunchKernelGGL(k_rescale_leaky_out_t, gt, dim3(kRrtBS), 0, st, ak, sa, lk, x, y, gtab, etab, mc);
        return;
    }
    launch_rescale_mrs_out(a, x, B, mc, g, st);
    launch_leaky_mult(sa, lk, x, y, gtab, etab, mc, st);
}

// Joint Clip: whether the planner defers the rescale's outputs to launch_rescale_clip_out. The joint-fuse mode
// forces it on (1) or off (0); in auto mode (-1) clip_fuse_pick decides: the launches that take the throughput
// kernel (batches of at least 3 GCs, staged shapes) from 2048 elements per GC, the smallest layer measured. The
// fused form won every alternation at N = 2048 .. 16384 and B = 3, 8, 24, 85 (profiles/ab/clip_joint/README.md:
// 10 - 22 % of the pair); nothing smaller was measured, so nothing smaller fuses. This is the Clip's own
// threshold, not kJointFuseMinElems.
constexpr int64_t kClipFuseMinN = 2048;
bool clip_fuse_pick(int64_t N, int B) { return B >= 3 && stage_ok(N, kRrtBS) && N >= kClipFuseMinN; }
bool clip_fuse(int64_t N, int B) {
    const int mode = joint_fuse_mode();
    return mode >= 0 ? mode == 1 : clip_fuse_pick(N, B);
}

// The deferred outputs of a rescale with a joint Clip behind it: the throughput form (k_rescale_clip_out_t) for
// batches of at least 3 GCs on staged shapes whose base fits its image; every other launch runs the rescale's
// output-hash kernel and the clip multiply, as the planner does without the fusion.
void launch_rescale_clip_out(const MrsArgs& a, const ClipArgs& ca, const Act& x, const Act& y, int B, const ModC* mc,
                             const AesGlobals& g, hipStream_t st) {
    if (B >= 3 && stage_ok(a.N, kRrtBS) && rrt_fits(a)) {
        const dim3 gt(static_cast<unsigned>((a.N + kRrtBS - 1) / kRrtBS), a.crt.k, B);
        if (launch_log_on()) launch_log_add("clip_out.tput", gt, dim3(kRrtBS));
        MrsArgs ak = a;
        ak.cmod = const_mod_on() ? 1 : 0;
        if (ak.cmod) const_mod_count(false);
        hipLaunchKernelGGL(k_rescale_clip_out_t, gt, dim3(kRrtBS), 0, st, ak, ca, x, y, mc);
        return;
    }
    launch_rescale_mrs_out(a, x, B, mc, g, st);
    launch_clip_mult(ca, x, y, B, mc, st);
}

// hx[b][j][e] = H(compress(x_j)), colx = color: the ReLU multiply's garbler half gates (exact-sign path;
// the approximate path gets them from k_sign_approx). grid (x, k, B)
__global__ __launch_bounds__(kAesBlock, kAesMinBlocks) void k_label_hash(Act x, CrtInfo crt, int64_t N, u128* hx,
                                                                        uint16_t* colx, const ModC* mc,
                                                                        const uint32_t* te0, const uint32_t* rk,
                                                                        int hard, uint64_t mgate0) {
    AES_PROLOGUE(te0, rk);
    const int j = blockIdx.y, b = blockIdx.z;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const ModC m = mc[crt.p[j]];
        const act_t* L = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
        const int64_t bke = (static_cast<int64_t>(b) * crt.k + j) * N + e;
        colx[bke] = static_cast<uint16_t>(static_cast<uint16_t>(L[0]) % m.q);
        const u128 C = compress_cm(L, N, m);
        hx[bke] = hard ? hard_pad(C, mgate0 ^ static_cast<uint64_t>(e), tw_sub(kTwMmg, j), 0) : aes_encrypt(aes, C);
    }
}

// the chain launch of CRT size a.crt.k (per-K units kernels_mrs_*.hip, mrs_chain.h)
static void dispatch_mrs_chain(const MrsArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g,
                               hipStream_t st) {
    switch (a.crt.k) {
        case 2: launch_mrs_chain_k<2>(a, x, B, mc, g, st); break;
        case 3: launch_mrs_chain_k<3>(a, x, B, mc, g, st); break;
        case 4: launch_mrs_chain_k<4>(a, x, B, mc, g, st); break;
        case 5: launch_mrs_chain_k<5>(a, x, B, mc, g, st); break;
        case 6: launch_mrs_chain_k<6>(a, x, B, mc, g, st); break;
        case 7: launch_mrs_chain_k<7>(a, x, B, mc, g, st); break;
        case 8: launch_mrs_chain_k<8>(a, x, B, mc, g, st); break;
        case 9: launch_mrs_chain_k<9>(a, x, B, mc, g, st); break;
        case 10: launch_mrs_chain_k<10>(a, x, B, mc, g, st); break;
        case 11: launch_mrs_chain_k<11>(a, x, B, mc, g, st); break;
        case 12: launch_mrs_chain_k<12>(a, x, B, mc, g, st); break;
        default: std::fprintf(stderr, "dash: mixed-radix chains support 2..12 CRT residues\n"); std::abort();
    }
}

void launch_relu_mrs(const MrsArgs& a, const SignArgs& sa, const Act& x, const Act& y, const u128* gtab,
                     const u128* etab, int B, const ModC* mc, const AesGlobals& g, hipStream_t st) {
    AES_LAUNCH_GGL(k_label_hash, a.N, a.crt.k, B, kAesLds, st, x, a.crt, a.N, sa.hx, sa.colx, mc, g.te0, g.rk,
                   sa.hard, sa.mgate0);
    dispatch_mrs_chain(a, x, B, mc, g, st);
    launch_relu_mult(sa, x, y, gtab, etab, mc, st);
}

void launch_leaky_mrs(const MrsArgs& a, const SignArgs& sa, const LeakyTab& lk, const Act& x, const Act& y,
                      const u128* gtab, const u128* etab, int B, const ModC* mc, const AesGlobals& g, hipStream_t st) {
    AES_LAUNCH_GGL(k_label_hash, a.N, a.crt.k, B, kAesLds, st, x, a.crt, a.N, sa.hx, sa.colx, mc, g.te0, g.rk,
                   sa.hard, sa.mgate0);
    dispatch_mrs_chain(a, x, B, mc, g, st);
    launch_leaky_mult(sa, lk, x, y, gtab, etab, mc, st);
}

// ReLU after a sign-producing rescale: the rescale wrote the sign's hash / color (chain MODE 2) and the
// half-gate keys of x (k_rescale_mrs_out_hash); only the mixed-modulus multiply is left
void launch_relu_joint(const SignArgs& sa, const Act& x, const Act& y, const u128* gtab, const u128* etab, int B,
                       const ModC* mc, const AesGlobals& g, hipStream_t st) {
    (void)B;
    (void)g;
    launch_relu_mult(sa, x, y, gtab, etab, mc, st);
}

// Quad form of k_rescale_mrs_out for latency-bound launches (batch 1, small layers): four lanes per (element,
// residue), the payload's chunks dealt over the quad (as k_rescale_relu_out_q's first pass), rows staged and
// stored as 16-byte units.
__global__ __launch_bounds__(256) void k_rescale_mrs_out_q(MrsArgs a, Act x, const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t sL[128 * kRroQE];
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int k = a.crt.k;
    const ModC m = mc[a.crt.p[j]];
    const int n = static_cast<int>(m.n);
    const int tid = static_cast<int>(threadIdx.x);
    const int el = tid >> 2, g = tid & 3;
    const uint32_t inv = static_cast<uint32_t>(a.sinv[j]);
    act_t* L = x.p[j] + static_cast<int64_t>(b) * n * N;
    for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRroQE; e0 < N; e0 += static_cast<int64_t>(gridDim.x) * kRroQE) {
        const int64_t e = min(e0 + el, N - 1);
        const u128 P = a.pf[(static_cast<int64_t>(b) * k + j) * N + e];
        __syncthreads();
        if (j != 0) quad_stage_rows(sL, L, N, e0, n);
        __syncthreads();
        quad_rescale_walk<kRroQE, false>(sL + el, n, g, P, inv, j == 0, m);
        __syncthreads();
        quad_store_rows(L, sL, N, e0, n);
    }
}

void launch_rescale_mrs(const MrsArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g, hipStream_t st,
                        bool chain_only) {
    dispatch_mrs_chain(a, x, B, mc, g, st);
    if (chain_only) return;  // the joint ReLU's k_rescale_relu_out writes the outputs
    launch_rescale_mrs_out(a, x, B, mc, g, st);
}

// The output kernels of a mixed-radix rescale whose chain has run (a.pf): split from the chain for a joint Clip,
// whose upper sign chain reads the rescale's input labels between the two.
void launch_rescale_mrs_out(const MrsArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g,
                            hipStream_t st) {
    if (a.mode == 2 && stage_ok(a.N, kOhBS)) {
        const dim3 gs = grid_aes(a.N, kOhBS, a.crt.k, B);
        if (launch_log_on()) launch_log_add("out_hash.staged", gs, dim3(kOhBS));
        hipLaunchKernelGGL(k_rescale_mrs_out_hash_s, gs, dim3(kOhBS), 0, st, a, x, mc, g.te0, g.rk);
    } else if (a.mode == 2) {
        const LaunchDims d = aes_dims("out_hash.lane", a.N, a.crt.k, B);
        hipLaunchKernelGGL(k_rescale_mrs_out_hash, d.grid, d.block, kAesLds, st, a, x, mc, g.te0, g.rk);
    } else if (out_quad_fits(a, B)) {
        const dim3 gq(static_cast<unsigned>((a.N + kRroQE - 1) / kRroQE), a.crt.k, B);
        if (launch_log_on()) launch_log_add("mrs_out.quad", gq, dim3(256));
        hipLaunchKernelGGL(k_rescale_mrs_out_q, gq, dim3(256), 0, st, a, x, mc);
    } else {
        const dim3 gl(static_cast<unsigned>((a.N + 255) / 256), a.crt.k, B);
        if (launch_log_on()) launch_log_add("mrs_out.lane", gl, dim3(256));
        hipLaunchKernelGGL(k_rescale_mrs_out, gl, dim3(256), 0, st, a, x, mc);
    }
}

// ---------------------------------------------------------------------------
// ReDash base extension (MRS conversion). One lane per (GC, element); the
// working copies live in `work` (component-major, [B][E][128][N]).

__global__ __launch_bounds__(256) void k_base_ext(BEArgs a, Act x, const ModC* mc, const uint32_t* te0,
                                                  const uint32_t* rk) {
    AES_PROLOGUE(te0, rk);
    const int b = blockIdx.z;
    const int64_t N = a.N;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int E = a.E;
    auto W = [&](int pos) { return a.work + ((static_cast<int64_t>(b) * E + pos) * 128) * N + e; };
    for (int i = 0; i < E; ++i) {
        const ModC m = mc[a.swapped[i]];
        const act_t* src = x.p[a.src[i]] + static_cast<int64_t>(b) * m.n * N + e;
        int16_t* w = W(i);
        col_map(src, w, N, static_cast<int>(m.n), [](int, int16_t v) { return v; });
    }
    const u128* T = a.tab + (static_cast<int64_t>(b) * N + e) * a.n_tab;
    int64_t off = 0;
    for (int i = 0; i < a.nonext; ++i) {
        const ModC mi = mc[a.swapped[i]];
        const int16_t* li = W(i);
        const u128 C = compress_cm(li, N, mi);
        const u128 H = a.hard ? 0 : aes_encrypt(aes, C);
        const uint32_t col = static_cast<uint16_t>(li[0]);
        for (int j = 0; j < E - i - 1; ++j) {
            const int tg = i + j + 1;
            const int q = a.swapped[tg];
            const ModC mo = mc[q];
            const u128 P = T[off + col] - (a.hard ? hard_pad(C, a.gate0 ^ static_cast<uint64_t>(e), tw_sub(kTwBe, i), j) : H);
            off += mi.q;
            DigitStream s;
            s.init(P);
            int16_t* lt = W(tg);
            const int32_t inv = a.inv[i][j];
            col_map(lt, lt, N, static_cast<int>(mo.n), [&](int, int16_t x) {
                int32_t v = x - static_cast<int32_t>(s.next(mo));
                if (v < 0) v += q;
                return static_cast<int16_t>(modq(static_cast<uint32_t>(v * inv), mo));
            });
        }
    }
    for (int xi = 0; xi < a.nextra; ++xi) {
        const int r = a.extra_res[xi];
        const int q = a.swapped[a.extra_pos[xi]];
        const ModC m = mc[q];
        const int16_t* w = W(a.extra_pos[xi]);
        act_t* dst = x.p[r] + static_cast<int64_t>(b) * m.n * N + e;
        const int32_t f = a.invv[xi];  // already negated mod q on the host
        col_map(w, dst, N, static_cast<int>(m.n), [&](int, int16_t v) { return static_cast<int16_t>(modq(static_cast<uint32_t>(v * f), m)); });
    }
    }
}

// ---------------------------------------------------------------------------
// Generic projection layer (test-only Projection). grid (ceil(N/256), k, B)
__global__ __launch_bounds__(kAesBlock, kAesMinBlocks) void k_proj(ProjArgs a, Act x, Act y, const ModC* mc, const uint32_t* te0,
                                              const uint32_t* rk) {
    AES_PROLOGUE(te0, rk);
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < N;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const ModC mi = mc[a.pin[j]], mo = mc[a.pout[j]];
    const act_t* L = x.p[j] + static_cast<int64_t>(b) * mi.n * N + e;
    const u128 C = compress_cm(L, N, mi);
    const u128 H = a.hard ? hard_pad(C, a.gate0 ^ static_cast<uint64_t>(e), tw_sub(kTwProj, j), 0) : aes_encrypt(aes, C);
    const uint32_t col = static_cast<uint16_t>(L[0]) % mi.q;
    const u128 P = a.tab[j][(static_cast<int64_t>(b) * N + e) * mi.q + col] - H;
    DigitStream s;
    s.init(P);
    act_t* O = y.p[j] + static_cast<int64_t>(b) * mo.n * N + e;
    for (int i = 0; i < static_cast<int>(mo.n); ++i) O[i * N] = static_cast<act_t>(s.next(mo));
    }
}

// Generalized half-gate product of pairs (2e, 2e+1), and the mixed-modulus
// variant (second operand first projected to Z_q). grid (ceil(No/256), k, B)
__global__ __launch_bounds__(kAesBlock, kAesMinBlocks) void k_mult(MultArgs a, Act x, Act y, const ModC* mc, const uint32_t* te0,
                                              const uint32_t* rk) {
    AES_PROLOGUE(te0, rk);
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t No = a.No, Ni = 2 * No;
    for (int64_t o = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; o < No;
         o += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * m.n * Ni + 2 * o;
    const act_t* Yv = X + 1;
    const int64_t bo = static_cast<int64_t>(b) * No + o;
    const uint64_t gt = a.gate0 ^ static_cast<uint64_t>(o);
    const u128 Cx = compress_cm(X, Ni, m);
    const u128 Hx = a.hard ? hard_pad(Cx, gt, tw_sub(kTwMmg, j), 0) : aes_encrypt(aes, Cx);
    const uint32_t colx = static_cast<uint16_t>(X[0]) % p;
    const u128 G = a.g[bo * a.crt.sum + a.crt.prefix[j] + colx] - Hx;
    u128 E;
    int32_t ypr;
    if (a.q == 0) {
        const u128 Cy = compress_cm(Yv, Ni, m);
        const u128 Hy = a.hard ? hard_pad(Cy, gt, tw_sub(kTwGme, j), 0) : aes_encrypt(aes, Cy);
        const uint32_t coly = static_cast<uint16_t>(Yv[0]) % p;
        E = a.e[bo * a.crt.sum + a.crt.prefix[j] + coly] - Hy;
        ypr = static_cast<int32_t>(coly);
    } else {
        const ModC mq = mc[a.q];
        const u128 Cy = compress_cm(Yv, Ni, m);
        const u128 Hy = a.hard ? hard_pad(Cy, gt, tw_sub(kTwMmt, j), 0) : aes_encrypt(aes, Cy);
        const uint32_t coly = static_cast<uint16_t>(Yv[0]) % p;
        const u128 Pt = a.t[bo * a.crt.sum + a.crt.prefix[j] + coly] - Hy;  // compressed label mod q
        u128 Ht, Hm;
        if (a.hard) {  // own row (TW_MMY, j): entry slot 0, mini lane 0 of slot 1
            u128 pd[4];
            hard_block(Pt, gt, tw_sub(kTwMmy, j), 0, pd);
            Ht = pd[0];
            Hm = pd[1];
        } else {
            Ht = Hm = aes_encrypt(aes, Pt);
        }
        const uint32_t colt = u128_mod(Pt, mq);
        const u128* E3 = a.e + (bo * a.crt.k + j) * (a.q + 1);
        E = E3[colt] - Ht;
        const int16_t t16 = static_cast<int16_t>(static_cast<uint16_t>(E3[a.q] >> (16 * colt)));
        ypr = static_cast<int16_t>(t16 - static_cast<int16_t>(static_cast<uint16_t>(Hm)));
        ypr %= p;
        if (ypr < 0) ypr += p;
    }
    DigitStream sg, se;
    sg.init(G);
    se.init(E);
    act_t* O = y.p[j] + static_cast<int64_t>(b) * m.n * No + o;
    const int n = static_cast<int>(m.n);
    for (int i0 = 0; i0 < n; i0 += kChunk) {
        int16_t xv[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u)
            if (i0 + u < n) xv[u] = X[(i0 + u) * Ni];
#pragma unroll
        for (int u = 0; u < kChunk; ++u)
            if (i0 + u < n) {
                const int32_t gv = static_cast<int32_t>(sg.next(m));
                const int32_t ev = static_cast<int32_t>(se.next(m));
                int32_t v = (ev + ypr * static_cast<int32_t>(xv[u]) - gv) % p;
                if (v < 0) v += p;
                O[(i0 + u) * No] = static_cast<act_t>(v);
            }
    }
    }
}

// ---------------------------------------------------------------------------
// Mul layer (gadgets.h MulPlan; kargs.h MulArgs): out_j = E + colour(y_j) x_j - G, the generalized half gates
// of x[e] and y[e / bc] under the output element's gate. Hardened only: no AES prologue, both pads are ChaCha
// pads derived here from the two compressed labels (rows (TW_MMG, j) of x and (TW_GME, j) of y), so no hash pass
// precedes the multiply. y is read for its compressed label and colour alone.
struct MulLane {
    u128 G, E;
    uint32_t ypr;
};
// The evaluator half gate's row and multiplier from y's column (HBM, stride Ny)
__device__ __forceinline__ void mul_y_ops(const MulArgs& a, const Act& ys, int j, int b, int64_t e, uint64_t gt,
                                          const ModC& m, MulLane& r) {
    const int64_t ey = a.bc ? e / a.bc : e;
    const act_t* Yl = ys.p[j] + static_cast<int64_t>(b) * m.n * a.Ny + ey;
    const uint32_t coly = Yl[0];
    const u128 Eraw = a.e[(static_cast<int64_t>(b) * a.N + e) * a.crt.sum + a.crt.prefix[j] + coly];
    const u128 Cy = compress_cm(Yl, a.Ny, m);
    r.E = Eraw - hard_pad(Cy, gt, tw_sub(kTwGme, j), 0);
    r.ypr = coly;
}

// grid (ceil(N/256), k, B)
__global__ __launch_bounds__(256) void k_mul(MulArgs a, Act x, Act ys, Act y, const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const uint64_t gt = a.gate0 ^ static_cast<uint64_t>(e);
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    const uint32_t colx = X[0];
    const u128 Graw = a.g[(static_cast<int64_t>(b) * N + e) * a.crt.sum + a.crt.prefix[j] + colx];
    MulLane c;
    mul_y_ops(a, ys, j, b, e, gt, m, c);
    c.G = Graw - hard_pad(compress_cm(X, N, m), gt, tw_sub(kTwMmg, j), 0);
    DigitStream sg, se;
    sg.init(c.G);
    se.init(c.E);
    col_walk<kChunk>(X, y.p[j] + static_cast<int64_t>(b) * m.n * N + e, N, static_cast<int>(m.n), [&](int, uint32_t xv) {
        const uint32_t g = sg.next(m);
        return mult_digit(se.next(m), c.ypr, xv, p, g, m);
    });
}

// k_mul with the labels staged in LDS (mult_grid; as k_relu_mult_s): a block = (256-element tile, residue j, GC b).
// The table gathers go out first (the two colours are one byte each from HBM), the block's x_j rows come in as
// 16-byte loads, a lane compresses its column from the image (x is read from HBM once, the lane form reads it
// twice), rewrites it in place and the block stores the rows as 16-byte stores. An elementwise y has x's layout: its
// tile passes through the same image first, for its compressed label alone. A broadcast y is never staged: the
// lanes of a channel read one column, which the cache serves. BC: a.bc != 0, one instantiation per path.
template <bool BC>
__global__ __launch_bounds__(kRmBS) void k_mul_s(MulArgs a, Act x, Act ys, Act y, const ModC* mc) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[128 * kRmBS];
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int tid = static_cast<int>(threadIdx.x);
    const int p = a.crt.p[j];
    const ModC m = mc[p];
    const int n = static_cast<int>(m.n);
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * n * N;
    const act_t* Ys = ys.p[j] + static_cast<int64_t>(b) * n * a.Ny;
    act_t* Y = y.p[j] + static_cast<int64_t>(b) * n * N;
    for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kRmBS; e0 < N; e0 += static_cast<int64_t>(gridDim.x) * kRmBS) {
        const int64_t e = min(e0 + tid, N - 1);  // lanes past the end redo the last element (their column is not stored)
        const uint64_t gt = a.gate0 ^ static_cast<uint64_t>(e);
        const int64_t ey = BC ? e / a.bc : e;
        const uint32_t colx = X[e], coly = Ys[ey];
        const int64_t row = (static_cast<int64_t>(b) * N + e) * a.crt.sum + a.crt.prefix[j];
        const u128 Graw = a.g[row + colx], Eraw = a.e[row + coly];
        u128 E;
        if (BC) E = Eraw - hard_pad(compress_cm(Ys + ey, a.Ny, m), gt, tw_sub(kTwGme, j), 0);
        __syncthreads();  // the previous tile's stores have read the image
        if (!BC) {  // Ny == N
            lds_stage_rows<kRmBS, 4, true>(stg, Ys, N, e0, 0, n);
            __syncthreads();
            const u128 Cy = compress_cm(stg + tid, kRmBS, m);
            __syncthreads();
            lds_stage_rows<kRmBS, 4, true>(stg, X, N, e0, 0, n);
            E = Eraw - hard_pad(Cy, gt, tw_sub(kTwGme, j), 0);  // while the other waves still stage
        } else {
            lds_stage_rows<kRmBS, 4, true>(stg, X, N, e0, 0, n);
        }
        __syncthreads();
        // a lane past the end compresses rows nobody staged: its keys, pads and column are never stored
        const u128 G = Graw - hard_pad(compress_cm(stg + tid, kRmBS, m), gt, tw_sub(kTwMmg, j), 0);
        lds_mult_walk<kRmBS, false>(stg + tid, n, G, E, 0, coly, p, m);
        __syncthreads();
        lds_store_rows<kRmBS>(Y, stg, N, e0, 0, n);
    }
}

// The square: one projection v -> v^2 per residue (rows (TW_PROJ, j)), k_proj's body with a ChaCha pad.
// grid (ceil(N/256), k, B)
__global__ __launch_bounds__(256) void k_mul_sq(MulArgs a, Act x, Act y, const ModC* mc) {
    const int j = blockIdx.y, b = blockIdx.z;
    const int64_t N = a.N;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const ModC m = mc[a.crt.p[j]];
    const act_t* X = x.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    const uint32_t colx = X[0];
    const u128 Traw = a.g[(static_cast<int64_t>(b) * N + e) * a.crt.sum + a.crt.prefix[j] + colx];
    const u128 H = hard_pad(compress_cm(X, N, m), a.gate0 ^ static_cast<uint64_t>(e), tw_sub(kTwProj, j), 0);
    DigitStream s;
    s.init(Traw - H);
    act_t* O = y.p[j] + static_cast<int64_t>(b) * m.n * N + e;
    for (int i = 0; i < static_cast<int>(m.n); ++i) O[static_cast<int64_t>(i) * N] = static_cast<act_t>(s.next(m));
}

// ---------------------------------------------------------------------------
// launchers
static inline dim3 grid_for(int64_t n, int bs, int y, int z) {
    return dim3(static_cast<unsigned>((n + bs - 1) / bs), y, z);
}


void launch_sign_approx(const SignArgs& a, const Act& x, const ModC* mc, const AesGlobals& g, hipStream_t st) {
    if (a.t <= 5)
        AES_LAUNCH_GGL(k_sign_approx<5>, a.N, a.crt.k, a.B, kAesLds, st, a, x, mc, g.te0, g.rk);
    else
        AES_LAUNCH_GGL(k_sign_approx<8>, a.N, a.crt.k, a.B, kAesLds, st, a, x, mc, g.te0, g.rk);
}
void launch_sign_chain(const SignArgs& a, int maxn, const ModC* mc, const AesGlobals& g, hipStream_t st) {
    const dim3 gs = grid_for(a.N, 256, a.t, a.B);
    const LaunchDims dr = aes_dims(a.fused ? "k_sign_chain_fused" : "k_sign_chain", a.N, 1, a.B);
    const dim3 gr = dr.grid, br = dr.block;
    // (measured: folding the castsum pass into the chain lanes is slower, 334 vs 356 inf/s on
    // MiniONN B=24: the chain is latency bound and the castsum's t-fold lane parallelism wins)
    if (maxn <= 24) {  // k = 7 DASH configs (cast outputs mod 8 m_d: <= 22 components)
        hipLaunchKernelGGL(k_sign_castsum<24>, gs, dim3(256), 0, st, a, mc);
        if (a.fused)
            hipLaunchKernelGGL(k_sign_chain_fused<24>, gr, br, kAesLds, st, a, mc, g.te0, g.rk);
        else
            hipLaunchKernelGGL(k_sign_chain<24>, gr, br, kAesLds, st, a, mc, g.te0, g.rk);
    } else if (maxn <= 32) {
        hipLaunchKernelGGL(k_sign_castsum<32>, gs, dim3(256), 0, st, a, mc);
        if (a.fused)
            hipLaunchKernelGGL(k_sign_chain_fused<32>, gr, br, kAesLds, st, a, mc, g.te0, g.rk);
        else
            hipLaunchKernelGGL(k_sign_chain<32>, gr, br, kAesLds, st, a, mc, g.te0, g.rk);
    } else {
        hipLaunchKernelGGL(k_sign_castsum<64>, gs, dim3(256), 0, st, a, mc);
        if (a.fused)
            hipLaunchKernelGGL(k_sign_chain_fused<64>, gr, br, kAesLds, st, a, mc, g.te0, g.rk);
        else
            hipLaunchKernelGGL(k_sign_chain<64>, gr, br, kAesLds, st, a, mc, g.te0, g.rk);
    }
}
void launch_unpack(const u128* P, int nres, const Act& out, const CrtInfo& mods, const ModC* mc, int64_t N, int B,
                   hipStream_t st) {
    hipLaunchKernelGGL(k_unpack, grid_for(N, 256, nres, B), dim3(256), 0, st, P, nres, out, mods, mc, N);
}
// The multiply's picker: the staged form (256-element tiles, kRmBS threads) where the shape allows and the
// output is apart from the input, a block striding over the tiles at 16 blocks per CU over the launch; else a
// lane per element (256 threads). Logs "<op>.staged" / "<op>.lane"; true for the staged form.
static bool mult_grid(const char* op, int64_t N, int k, int B, const Act& x, const Act& y, dim3& grid) {
    const bool staged = stage_ok(N, kRmBS) && x.p[0] != y.p[0];
    grid = grid_for(N, 256, k, B);
    if (staged) grid.x = static_cast<unsigned>(std::min<int64_t>((N + kRmBS - 1) / kRmBS, std::max(1, 16 * num_cus() / (k * B))));
    if (launch_log_on()) launch_log_add(std::string(op) + (staged ? ".staged" : ".lane"), grid, dim3(staged ? kRmBS : 256));
    return staged;
}
void launch_relu_mult(const SignArgs& a, const Act& x, const Act& y, const u128* gtab, const u128* etab,
                      const ModC* mc, hipStream_t st) {
    dim3 grid;
    if (mult_grid("relu_mult", a.N, a.crt.k, a.B, x, y, grid))
        hipLaunchKernelGGL(k_relu_mult_s, grid, dim3(kRmBS), 0, st, a, x, y, gtab, etab, mc);
    else
        hipLaunchKernelGGL(k_relu_mult, grid, dim3(256), 0, st, a, x, y, gtab, etab, mc);
}
void launch_leaky_mult(const SignArgs& a, const LeakyTab& lk, const Act& x, const Act& y, const u128* gtab,
                       const u128* etab, const ModC* mc, hipStream_t st) {
    dim3 grid;
    if (mult_grid("leaky_mult", a.N, a.crt.k, a.B, x, y, grid))
        hipLaunchKernelGGL(k_leaky_mult_s, grid, dim3(kRmBS), 0, st, a, lk, x, y, gtab, etab, mc);
    else
        hipLaunchKernelGGL(k_leaky_mult, grid, dim3(256), 0, st, a, lk, x, y, gtab, etab, mc);
}
// Clip: the half gates' keys of x (as launch_relu_mrs), then one sign per bound into its own scratch, then the
// multiply. The multiply's picker is launch_relu_mult's (mult_grid).
void launch_clip_hash(const ClipArgs& a, u128* hx, uint16_t* colx, const Act& x, int B, const ModC* mc,
                      const AesGlobals& g, hipStream_t st) {
    AES_LAUNCH_GGL(k_label_hash, a.N, a.crt.k, B, kAesLds, st, x, a.crt, a.N, hx, colx, mc, g.te0, g.rk, 1, a.mgate0);
}
void launch_clip_sign_mrs(const MrsArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g, hipStream_t st) {
    dispatch_mrs_chain(a, x, B, mc, g, st);
}
void launch_clip_mult(const ClipArgs& a, const Act& x, const Act& y, int B, const ModC* mc, hipStream_t st) {
    dim3 grid;
    if (mult_grid("clip_mult", a.N, a.crt.k, B, x, y, grid))
        hipLaunchKernelGGL(k_clip_mult_s, grid, dim3(kRmBS), 0, st, a, x, y, mc);
    else
        hipLaunchKernelGGL(k_clip_mult, grid, dim3(256), 0, st, a, x, y, mc);
}
// PiecewiseLinear: the compressed labels of x once, then (after the m sign launches, each into its own key
// buffer) the multiply, instantiated per kept-breakpoint count. The picker is launch_relu_mult's (mult_grid).
void launch_pwl_key(const PwlArgs& a, u128* kx, uint16_t* colx, const Act& x, int B, const ModC* mc, hipStream_t st) {
    hipLaunchKernelGGL(k_label_key, grid_for(a.N, 256, a.crt.k, B), dim3(256), 0, st, x, a.crt, a.N, kx, colx, mc);
}
void launch_label_key(const CrtInfo& crt, int64_t N, u128* kx, uint16_t* colx, const Act& x, int B, const ModC* mc,
                      hipStream_t st) {
    hipLaunchKernelGGL(k_label_key, grid_for(N, 256, crt.k, B), dim3(256), 0, st, x, crt, N, kx, colx, mc);
}
template <int M>
static void launch_pwl_mult_m(const PwlArgs& a, const Act& x, const Act& y, int B, const ModC* mc, hipStream_t st) {
    dim3 grid;
    if (mult_grid("pwl_mult", a.N, a.crt.k, B, x, y, grid))
        hipLaunchKernelGGL(k_pwl_mult_s<M>, grid, dim3(kRmBS), 0, st, a, x, y, mc);
    else
        hipLaunchKernelGGL(k_pwl_mult<M>, grid, dim3(256), 0, st, a, x, y, mc);
}
void launch_pwl_mult(const PwlArgs& a, const Act& x, const Act& y, int B, const ModC* mc, hipStream_t st) {
    switch (a.m) {
        case 1: launch_pwl_mult_m<1>(a, x, y, B, mc, st); break;
        case 2: launch_pwl_mult_m<2>(a, x, y, B, mc, st); break;
        case 3: launch_pwl_mult_m<3>(a, x, y, B, mc, st); break;
        case 4: launch_pwl_mult_m<4>(a, x, y, B, mc, st); break;
        case 5: launch_pwl_mult_m<5>(a, x, y, B, mc, st); break;
        case 6: launch_pwl_mult_m<6>(a, x, y, B, mc, st); break;
        case 7: launch_pwl_mult_m<7>(a, x, y, B, mc, st); break;
        case 8: launch_pwl_mult_m<8>(a, x, y, B, mc, st); break;
        default: std::fprintf(stderr, "dash: a PiecewiseLinear layer has 1..8 breakpoints\n"); std::abort();
    }
}
// ArgMax (gadgets.h ArgMaxPlan), per level: the pair differences, the half gates' keys of a difference under one
// gate set's gate, the sign chain (launch_clip_sign_mrs) and the multiply, whose form is the level's shape.
void launch_argmax_diff(const Act& v, const Act& d, int64_t P, int ops, int cnt, int pubq, const CrtInfo& crt, int B,
                        hipStream_t st) {
    int nmax = 1;
    for (int j = 0; j < crt.k; ++j) nmax = std::max(nmax, crt.n[j]);
    hipLaunchKernelGGL(k_argmax_diff, grid_for(P * ops * nmax, 256, crt.k, B), dim3(256), 0, st, v, d, P, ops, cnt, pubq,
                       crt);
}
void launch_argmax_hash(const Act& d, const CrtInfo& crt, int64_t N, u128* hx, uint16_t* colx, uint64_t gate0, int B,
                        const ModC* mc, const AesGlobals& g, hipStream_t st) {
    AES_LAUNCH_GGL(k_label_hash, N, crt.k, B, kAesLds, st, d, crt, N, hx, colx, mc, g.te0, g.rk, 1, gate0);
}
void launch_argmax_mult(const ArgMaxArgs& a, bool val, bool l0, const Act& v, const Act& d, const Act& i, const Act& ed,
                        const Act& nv, const Act& ni, int B, const ModC* mc, hipStream_t st) {
    const dim3 grid = grid_for(a.P * a.ops, 256, a.crt.k, B);
    if (launch_log_on())
        launch_log_add(std::string("argmax_mult.") + (l0 ? (val ? "l0" : "root0") : (val ? "mid" : "root")), grid, dim3(256));
    if (val && l0) hipLaunchKernelGGL((k_argmax_mult<true, true>), grid, dim3(256), 0, st, a, v, d, i, ed, nv, ni, mc);
    else if (val) hipLaunchKernelGGL((k_argmax_mult<true, false>), grid, dim3(256), 0, st, a, v, d, i, ed, nv, ni, mc);
    else if (l0) hipLaunchKernelGGL((k_argmax_mult<false, true>), grid, dim3(256), 0, st, a, v, d, i, ed, nv, ni, mc);
    else hipLaunchKernelGGL((k_argmax_mult<false, false>), grid, dim3(256), 0, st, a, v, d, i, ed, nv, ni, mc);
}
void launch_rescale_hash(const Act& x, int fi, int s, const int16_t* up, int up_stride, int add_up, int64_t N, int B,
                         u128* h0, uint16_t* col0, const ModC* mc, const AesGlobals& g, hipStream_t st, int hard) {
    AES_LAUNCH_GGL(k_rescale_hash, N, 1, B, kAesLds, st, x, fi, s, up, up_stride, add_up, N, h0, col0, mc, g.te0,
                   g.rk, hard);
}
void launch_rescale_update(const RescaleArgs& a, const Act& x, int B, const ModC* mc, hipStream_t st) {
    hipLaunchKernelGGL(k_rescale_update, grid_for(a.N, 256, a.crt.k, B), dim3(256), 0, st, a, x, mc);
}
void launch_rescale_post(const Act& x, const CrtInfo& crt, int64_t N, int B, const u128* signP, const int16_t* down,
                         int lab_stride, const int* lab_off, const ModC* mc, hipStream_t st) {
    hipLaunchKernelGGL(k_rescale_post, grid_for(N, 256, crt.k, B), dim3(256), 0, st, x, crt, N, signP, down,
                       lab_stride, lab_off, mc);
}
void launch_base_ext(const BEArgs& a, const Act& x, int B, const ModC* mc, const AesGlobals& g, hipStream_t st) {
    hipLaunchKernelGGL(k_base_ext, grid_aes(a.N, 256, 1, B), dim3(256), kAesLds, st, a, x, mc, g.te0, g.rk);
}
void launch_proj(const ProjArgs& a, const Act& x, const Act& y, int B, const ModC* mc, const AesGlobals& g,
                 hipStream_t st) {
    AES_LAUNCH_GGL(k_proj, a.N, a.k, B, kAesLds, st, a, x, y, mc, g.te0, g.rk);
}
void launch_mul(const MulArgs& a, bool square, const Act& x, const Act& ys, const Act& y, int B, const ModC* mc,
                hipStream_t st) {
    if (square) {
        const dim3 grid = grid_for(a.N, 256, a.crt.k, B);
        if (launch_log_on()) launch_log_add("mul.sq", grid, dim3(256));
        hipLaunchKernelGGL(k_mul_sq, grid, dim3(256), 0, st, a, x, y, mc);
        return;
    }
    dim3 grid;
    if (mult_grid("mul", a.N, a.crt.k, B, x, y, grid)) {
        if (a.bc) hipLaunchKernelGGL(k_mul_s<true>, grid, dim3(kRmBS), 0, st, a, x, ys, y, mc);
        else hipLaunchKernelGGL(k_mul_s<false>, grid, dim3(kRmBS), 0, st, a, x, ys, y, mc);
    } else
        hipLaunchKernelGGL(k_mul, grid, dim3(256), 0, st, a, x, ys, y, mc);
}
void launch_mult(const MultArgs& a, const Act& x, const Act& y, int B, const ModC* mc, const AesGlobals& g,
                 hipStream_t st) {
    AES_LAUNCH_GGL(k_mult, a.No, a.crt.k, B, kAesLds, st, a, x, y, mc, g.te0, g.rk);
}

}  // namespace dev
}  // namespace dash
