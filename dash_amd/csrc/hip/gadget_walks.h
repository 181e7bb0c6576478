// The half-gate operands and the column walks shared by the ReLU / Clip multiply, the mixed-radix rescale output
// and their fused forms (kernels_gadget.hip only): relu_j = E + ypr x_j - G (+ C), Y_j = S^-1 L_j + digits(P).
// A walk rewrites one element's column of a component-major label: in HBM (stride N, one byte per lane per
// access) or in an LDS image S[c][BS] (the caller passes its own column, S + tid).
#pragma once

#include "gadget_common.h"

namespace dash {
namespace dev {

// ---------------------------------------------------------------------------
// Half-gate operands.

// The evaluator half gate's multiplier ypr in [0, p): lane `colour` of the mini gate minus the low 16 bits of
// its pad HM, a signed 16-bit difference d (the garbler's ypr16). p * 2^15 > |d|, so the shifted sum is
// positive and one reduction gives d mod p.
__device__ __forceinline__ uint32_t mini_mult(u128 mini, uint32_t colour, u128 HM, int p, const ModC& m) {
    const int16_t t16 = static_cast<int16_t>(static_cast<uint16_t>(mini >> (16 * colour)));
    const int16_t d = static_cast<int16_t>(t16 - static_cast<int16_t>(static_cast<uint16_t>(HM)));
    return modq(static_cast<uint32_t>(static_cast<int32_t>(d) + (p << 15)), m);
}

// The ReLU evaluator half gate's gathers for (GC b, residue j, element e): the pads HS (entry) and HM (mini),
// the sign's colour cS, the entry Eraw = E3[cS] and the mini gate. Hardened (hs == nullptr): entry j under
// y-row pad j, mini j under lane j % 8 of pad k + j / 8 (MMTw, gadgets.h; chain MODE 2 store_ypads). Reference
// construction: the one H(sign label) hs[b][e] masks all k entries and minis.
struct ReluOps {
    u128 HS, HM, Eraw, mini;
    uint32_t cS;
};
__device__ __forceinline__ ReluOps relu_ops(const u128* hs, const u128* ys, int ny, const uint8_t* cs,
                                            const u128* etab, int b, int j, int k, int64_t N, int64_t e) {
    const int64_t be = static_cast<int64_t>(b) * N + e;
    ReluOps o;
    o.HS = hs ? hs[be] : ys[(static_cast<int64_t>(b) * ny + j) * N + e];
    o.HM = hs ? o.HS : (ys[(static_cast<int64_t>(b) * ny + k + j / 8) * N + e] >> (16 * (j % 8)));
    o.cS = cs[be];
    const u128* E3 = etab + (be * k + j) * 3;
    o.Eraw = E3[o.cS];
    o.mini = E3[2];
    return o;
}

// The same operands from the compressed mod-2 label Y itself (a Clip's u, an ArgMax's s), which keys residue
// j's evaluator half gate E3 = [k][3] under `gate`: the lane derives Y's y-row pads (TW_MMY, 0: entry slot j,
// mini lane j % 8 of slot k + j / 8). j is uniform per block, so is the choice of one or two pad blocks.
struct KeyedOps {
    u128 E;        // the entry of Y's colour minus its pad
    uint32_t ypr;  // the half gate's multiplier
};
__device__ __forceinline__ KeyedOps keyed_ops(u128 Y, uint64_t gate, const u128* E3, int j, int k, int p, const ModC& m) {
    const uint32_t cY = static_cast<uint32_t>(Y) & 1u;
    const u128 Eraw = E3[cY];
    const u128 mini = E3[2];
    const int sS = j, sM = k + j / 8;
    u128 pd[4];
    hard_block(Y, gate, tw_sub(kTwMmy, 0), static_cast<uint32_t>(sS) >> 2, pd);
    const u128 HS = pd[sS & 3];
    if ((sM >> 2) != (sS >> 2)) hard_block(Y, gate, tw_sub(kTwMmy, 0), static_cast<uint32_t>(sM) >> 2, pd);
    const u128 HM = pd[sM & 3] >> (16 * (j % 8));
    KeyedOps r;
    r.E = Eraw - HS;
    r.ypr = mini_mult(mini, cY, HM, p, m);
    return r;
}

// One digit of the multiply; all terms in [0, p): ev + ypr x + (p - g) (+ cv) < p^2 + 3p
__device__ __forceinline__ uint32_t mult_digit(uint32_t ev, uint32_t ypr, uint32_t x, int p, uint32_t g, const ModC& m) {
    return modq(ev + ypr * x + static_cast<uint32_t>(p) - g, m);
}

// LeakyRelu (gadgets.h LeakyPlan): a lane's two public factors, b = n_c mod p and c = (2^s - n_c) mod p, read
// once per lane from the layer's table [channel][residue] (b | c << 8), channel = e / bc.
struct LeakyLane {
    uint32_t fb, fc;
};
__device__ __forceinline__ LeakyLane leaky_lane(const LeakyTab& lk, int64_t e, int j, int k) {
    const uint32_t ch = static_cast<uint32_t>(e) / lk.bc;  // N < 2^32 (plan_leaky)
    const uint32_t v = lk.t[static_cast<int64_t>(ch) * k + j];
    return LeakyLane{v & 0xffu, v >> 8};
}
// The x multiplier of a leaky digit, folded once per lane: yl = (c ypr + b) mod p; c ypr + b < p^2
__device__ __forceinline__ uint32_t leaky_mult(uint32_t ypr, const LeakyLane& l, const ModC& m) {
    return modq(l.fc * ypr + l.fb, m);
}
// One digit of the leaky multiply: b x + c t with the ReLU digit t = ev + ypr x - g, computed as
// c (ev + p - g) + yl x in one reduction. All of ev, g, x, c, yl in [0, p), so the sum stays below
// (p - 1)(2p - 1) + (p - 1)^2 = (p - 1)(3p - 2): outside mult_digit's p^2 + 3p, inside the range in which modq's
// reciprocal (one correction) is exact, x < 2^32. tests/test_leaky_relu.py checks this formula with the same
// constants for every prime <= 37 and all operand values.
__device__ __forceinline__ uint32_t leaky_digit(uint32_t ev, uint32_t yl, uint32_t x, int p, uint32_t g, uint32_t fc,
                                                const ModC& m) {
    return modq(fc * (ev + static_cast<uint32_t>(p) - g) + yl * x, m);
}

// PiecewiseLinear (gadgets.h PwlPlan): one digit of a0 x + sum_i d_i t_i with the ReLU digits
// t_i = ev_i + ypr_i x - g_i, computed as yl x + sum_i d_i (ev_i + p - g_i) with the x multiplier folded once per
// lane, yl = (a0 + sum_i d_i ypr_i) mod p, accumulated unreduced and reduced once. All of ev, g, x, d, yl lie in
// [0, p), so with M <= 8 the sum stays below (p - 1)^2 + 8 (p - 1)(2p - 1) (22320 at p = 37): far inside the
// range in which modq's reciprocal (one correction) is exact. tests/test_pwl.py checks the formula and modq on
// the whole range with the same constants for every prime of the shipped bases.
template <int M>
struct PwlLane {
    u128 G[M], E[M];  // the garbler / evaluator half gates' rows minus their pads, per breakpoint
    uint32_t d[M];    // D_i mod p
    uint32_t yl;      // the folded x multiplier
};
template <int M, class FG, class FE>
__device__ __forceinline__ uint32_t pwl_digit(uint32_t x, const PwlLane<M>& l, int p, const ModC& m, FG&& g, FE&& ev) {
    uint32_t acc = l.yl * x;
#pragma unroll
    for (int i = 0; i < M; ++i) acc += l.d[i] * (ev(i) + static_cast<uint32_t>(p) - g(i));
    return modq(acc, m);
}
// p = 2: (a0 & x) ^ XOR_i (d_i & (e_i ^ g_i ^ (ypr_i & x))) = W ^ (yl & x) per bit with one word
// W = XOR_i (d_i ? G_i ^ E_i : 0)
template <int M>
__device__ __forceinline__ u128 pwl_bit_word(const PwlLane<M>& l) {
    u128 W = 0;
#pragma unroll
    for (int i = 0; i < M; ++i) W ^= (l.d[i] & 1u) ? (l.G[i] ^ l.E[i]) : static_cast<u128>(0);
    return W;
}

// ---------------------------------------------------------------------------
// Per-lane HBM column walk: dst[c * N] = f(c, src[c * N]) for c < n in component order, G components per round
// trip (dst may alias src). The loads of group c+1 go out before the stores of group c: vmcnt retires in issue
// order, so a load issued after a store would also wait for that store.
template <int G, class F>
__device__ __forceinline__ void col_walk(const act_t* src, act_t* dst, int64_t N, int n, F&& f) {
    uint16_t cur[G], nxt[G];
#pragma unroll
    for (int u = 0; u < G; ++u)
        if (u < n) cur[u] = src[static_cast<int64_t>(u) * N];
    for (int c0 = 0; c0 < n; c0 += G) {
#pragma unroll
        for (int u = 0; u < G; ++u)
            if (c0 + G + u < n) nxt[u] = src[static_cast<int64_t>(c0 + G + u) * N];
#pragma unroll
        for (int u = 0; u < G; ++u)
            if (c0 + u < n) dst[static_cast<int64_t>(c0 + u) * N] = static_cast<act_t>(f(c0 + u, static_cast<uint32_t>(cur[u])));
#pragma unroll
        for (int u = 0; u < G; ++u) cur[u] = nxt[u];
    }
}

// The same walk over NS source columns with a stride each (an ArgMax's pair operands live in buffers of
// different slot counts): f(c, v) gets component c of every source and does its own stores.
template <int G, int NS, class F>
__device__ __forceinline__ void col_walk_n(const act_t* const (&src)[NS], const int64_t (&ld)[NS], int n, F&& f) {
    uint16_t cur[NS][G], nxt[NS][G];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int u = 0; u < G; ++u)
            if (u < n) cur[s][u] = src[s][static_cast<int64_t>(u) * ld[s]];
    for (int c0 = 0; c0 < n; c0 += G) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int u = 0; u < G; ++u)
                if (c0 + G + u < n) nxt[s][u] = src[s][static_cast<int64_t>(c0 + G + u) * ld[s]];
#pragma unroll
        for (int u = 0; u < G; ++u)
            if (c0 + u < n) {
                uint32_t v[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) v[s] = cur[s][u];
                f(c0 + u, v);
            }
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int u = 0; u < G; ++u) cur[s][u] = nxt[s][u];
    }
}

// ---------------------------------------------------------------------------
// LDS column walks (col = the lane's column of an image of BS-byte rows).

// p = 2: a label's digits are the bits of its 128-bit word. Row c < cnt <= 128 becomes f(bit c of W, row c):
// one bit extract and the logic of f per component instead of a 128-bit digit shift and a reduction.
template <int BS, class F>
__device__ __forceinline__ void lds_bit_rows(uint8_t* col, int cnt, u128 W, F&& f) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t ww = static_cast<uint32_t>(W >> (32 * w));
#pragma unroll 8
        for (int u = 0; u < 32; ++u) {
            const int c = 32 * w + u;
            if (c >= cnt) break;
            uint8_t& v = col[c * BS];
            v = static_cast<uint8_t>(f((ww >> u) & 1u, static_cast<uint32_t>(v)));
        }
    }
}

// Chunk-major multiply walk (odd moduli, chunk_digit): one divmod per stream per chunk, uniform digit loops.
// CLIP adds the cap row's stream C. LEAKY: the digit becomes b x + c t (leaky_digit; no Clip form).
template <int BS, bool CLIP, bool LEAKY = false>
__device__ __forceinline__ void lds_mult_chunks(uint8_t* col, int n, u128 G, u128 E, u128 C, uint32_t ypr, int p,
                                                const ModC& m, LeakyLane lk = LeakyLane{0u, 0u}) {
    static_assert(!(CLIP && LEAKY), "no leaky Clip");
    const int c = static_cast<int>(m.c);
    const uint32_t yl = LEAKY ? leaky_mult(ypr, lk, m) : 0u;
    for (int k0 = 0; k0 < n; k0 += c) {
        uint32_t rg = divmod128(G, m), re = divmod128(E, m), rc = CLIP ? divmod128(C, m) : 0u;
        const int kc = min(c, n - k0);
#pragma unroll 4
        for (int t = 0; t < kc; ++t) {
            const uint32_t g = chunk_digit(rg, m);
            const uint32_t ev = chunk_digit(re, m) + (CLIP ? chunk_digit(rc, m) : 0u);
            uint8_t& v = col[(k0 + t) * BS];
            if (LEAKY)
                v = static_cast<uint8_t>(leaky_digit(ev, yl, v, p, g, lk.fc, m));
            else
                v = static_cast<uint8_t>(mult_digit(ev, ypr, v, p, g, m));
        }
    }
}

// The staged multiply of a whole column, in place: p = 2 as bit logic ((e + ypr x + 2 - g + c) mod 2 =
// e ^ g ^ c ^ (ypr & x); the residue with the most components, 128), other power-of-two moduli as digit
// streams, odd moduli chunk-major. LEAKY: b x + c t per digit, p = 2 still bit logic, (b & x) ^ (c & t).
template <int BS, bool CLIP, bool LEAKY = false>
__device__ __forceinline__ void lds_mult_walk(uint8_t* col, int n, u128 G, u128 E, u128 C, uint32_t ypr, int p,
                                              const ModC& m, LeakyLane lk = LeakyLane{0u, 0u}) {
    static_assert(!(CLIP && LEAKY), "no leaky Clip");
    if (m.bits == 1) {
        if (LEAKY)
            lds_bit_rows<BS>(col, n, G ^ E, [=](uint32_t bit, uint32_t x) {
                return (lk.fb & x) ^ (lk.fc & (bit ^ (x & ypr)));
            });
        else
            lds_bit_rows<BS>(col, n, CLIP ? G ^ E ^ C : G ^ E, [=](uint32_t bit, uint32_t x) { return bit ^ (x & ypr); });
    } else if (m.bits) {
        DigitStream sg, se, sc;
        sg.init(G);
        se.init(E);
        sc.init(C);
        const uint32_t yl = LEAKY ? leaky_mult(ypr, lk, m) : 0u;
        for (int c = 0; c < n; ++c) {
            const uint32_t g = sg.next(m);
            const uint32_t ev = se.next(m) + (CLIP ? sc.next(m) : 0u);
            uint8_t& v = col[c * BS];
            if (LEAKY)
                v = static_cast<uint8_t>(leaky_digit(ev, yl, v, p, g, lk.fc, m));
            else
                v = static_cast<uint8_t>(mult_digit(ev, ypr, v, p, g, m));
        }
    } else {
        lds_mult_chunks<BS, CLIP, LEAKY>(col, n, G, E, C, ypr, p, m, lk);
    }
}

// The staged PiecewiseLinear multiply of a whole column, in place (pwl_digit): p = 2 as bit logic on one word,
// other power-of-two moduli as digit streams, odd moduli chunk-major with one divmod per stream per chunk.
template <int BS, int M>
__device__ __forceinline__ void lds_pwl_walk(uint8_t* col, int n, PwlLane<M>& l, int p, const ModC& m) {
    if (m.bits == 1) {
        const uint32_t yl = l.yl & 1u;
        lds_bit_rows<BS>(col, n, pwl_bit_word(l), [=](uint32_t bit, uint32_t x) { return bit ^ (x & yl); });
    } else if (m.bits) {
        DigitStream sg[M], se[M];
#pragma unroll
        for (int i = 0; i < M; ++i) {
            sg[i].init(l.G[i]);
            se[i].init(l.E[i]);
        }
        for (int c = 0; c < n; ++c) {
            uint8_t& v = col[c * BS];
            v = static_cast<uint8_t>(pwl_digit(v, l, p, m, [&](int i) { return sg[i].next(m); },
                                               [&](int i) { return se[i].next(m); }));
        }
    } else {
        const int c = static_cast<int>(m.c);
        for (int k0 = 0; k0 < n; k0 += c) {
            uint32_t rg[M], re[M];
#pragma unroll
            for (int i = 0; i < M; ++i) {
                rg[i] = divmod128(l.G[i], m);
                re[i] = divmod128(l.E[i], m);
            }
            const int kc = min(c, n - k0);
            for (int t = 0; t < kc; ++t) {
                uint8_t& v = col[(k0 + t) * BS];
                v = static_cast<uint8_t>(pwl_digit(v, l, p, m, [&](int i) { return chunk_digit(rg[i], m); },
                                                   [&](int i) { return chunk_digit(re[i], m); }));
            }
        }
    }
}

// Chunk-major rescale walk with the key summed per chunk: rows [0, cnt) of col become Y = S^-1 L + digits of Q
// (payload: the digits alone, residue 0) and C gathers compress(Y), one flush per chunk. The state runs on
// over the passes of a label walked in windows of whole chunks. The digit loop is unrolled by 4 and the caller
// reads the first digit back after the pass instead of a compare per digit: the loop's scalar bookkeeping was
// ~40 % of the kernel's instructions (r05 headline PMC).
struct ChunkKey {
    u128 Q, C, PW;
    __device__ __forceinline__ void init(u128 P) {
        Q = P;
        C = 0;
        PW = 1;
    }
    template <int BS>
    __device__ __forceinline__ void walk(uint8_t* col, int cnt, uint32_t inv, bool payload, const ModC& m) {
        const int c = static_cast<int>(m.c);
        for (int k0 = 0; k0 < cnt; k0 += c) {
            uint32_t r = divmod128(Q, m);
            const int kc = min(c, cnt - k0);
            uint32_t acc = 0, pt = 1;
#pragma unroll 4
            for (int t = 0; t < kc; ++t) {
                uint8_t& w = col[(k0 + t) * BS];
                const uint32_t dd = chunk_digit(r, m);
                const uint32_t v = payload ? dd : modq(static_cast<uint32_t>(w) * inv + dd, m);  // < p^2 + p
                w = static_cast<uint8_t>(v);
                acc += v * pt;
                pt *= m.q;
            }
            C += PW * static_cast<u128>(acc);
            PW *= static_cast<u128>(m.D);
        }
    }
};

// ---------------------------------------------------------------------------
// Constant-modulus forms of the two chunk-major walks above (MK = ModK<p>, dev.h), for kernels whose block knows
// its residue: the label width, the chunk length and the last chunk's length are constants, so the chunk loop
// stays rolled and a chunk's digits are written out with no loop bookkeeping, two digits per extraction. The
// same digits, rows and key as ChunkKey::walk / lds_mult_chunks (tests/test_gpu_const_mod.py).

// rows [0, CNT) of col: one chunk of ChunkKey::walk (not payload); returns the chunk's value sum_t Y_t Q^t
template <class MK, int BS, int CNT>
__device__ __forceinline__ uint32_t rescale_chunk_k(uint8_t* col, uint32_t r, uint32_t inv) {
    typename MK::template Acc<CNT> acc;
    static_for<0, (CNT + 1) / 2>([&](auto tt) __attribute__((always_inline)) {
        constexpr int t = 2 * decltype(tt)::value;
        uint32_t p0, p1 = 0;
        if constexpr (t + 1 < CNT) MK::digit2(r, p0, p1);
        else p0 = MK::digit(r);
        // S^-1 L + digit < (Q - 1)^2 + Q
        const uint32_t v0 = MK::template mod<MK::QQ + 3 * MK::q>(__umul24(col[t * BS], inv) + p0);
        col[t * BS] = static_cast<uint8_t>(v0);
        acc.template push<t>(v0);
        if constexpr (t + 1 < CNT) {
            const uint32_t v1 = MK::template mod<MK::QQ + 3 * MK::q>(__umul24(col[(t + 1) * BS], inv) + p1);
            col[(t + 1) * BS] = static_cast<uint8_t>(v1);
            acc.template push<t + 1>(v1);
        }
        pair_fence();
    });
    return acc.value();
}
// ChunkKey::walk over a whole label of MK::n rows; returns the key compress(Y)
template <class MK, int BS>
__device__ __forceinline__ u128 rescale_walk_k(uint8_t* col, u128 P, uint32_t inv) {
    constexpr int c = static_cast<int>(MK::c), n = static_cast<int>(MK::n), nfull = n / c, tail = n % c;
    u128 C = 0, PW = 1;
#pragma unroll 1
    for (int ch = 0; ch < nfull; ++ch) {
        const uint32_t r = MK::divmod(P);
        C += PW * static_cast<u128>(rescale_chunk_k<MK, BS, c>(col + ch * c * BS, r, inv));
        PW *= static_cast<u128>(MK::D);
    }
    if constexpr (tail > 0) {
        const uint32_t r = MK::divmod(P);
        C += PW * static_cast<u128>(rescale_chunk_k<MK, BS, tail>(col + nfull * c * BS, r, inv));
    }
    return C;
}
// rows [0, CNT) of col: one chunk of lds_mult_chunks. The digit sums stay below the bounds of mult_digit
// (Q^2 + 3 Q, the Clip's second entry digit included) and leaky_digit ((Q - 1)(3 Q - 2)).
template <class MK, int BS, int CNT, bool CLIP, bool LEAKY>
__device__ __forceinline__ void mult_chunk_k(uint8_t* col, uint32_t rg, uint32_t re, uint32_t rc, uint32_t ypr,
                                             uint32_t yl, uint32_t fc) {
    constexpr uint32_t Q = MK::q;
    auto one = [&](uint8_t& w, uint32_t g, uint32_t ev) {
        const uint32_t x = w;
        if constexpr (LEAKY)
            w = static_cast<uint8_t>(MK::template mod<(Q - 1) * (3 * Q - 2) + 1>(__umul24(fc, ev + Q - g) + __umul24(yl, x)));
        else
            w = static_cast<uint8_t>(MK::template mod<MK::QQ + 3 * Q>(ev + __umul24(ypr, x) + Q - g));
    };
    static_for<0, (CNT + 1) / 2>([&](auto tt) __attribute__((always_inline)) {
        constexpr int t = 2 * decltype(tt)::value;
        uint32_t g0, g1 = 0, e0, e1 = 0, c0 = 0, c1 = 0;
        if constexpr (t + 1 < CNT) {
            MK::digit2(rg, g0, g1);
            MK::digit2(re, e0, e1);
            if constexpr (CLIP) MK::digit2(rc, c0, c1);
        } else {
            g0 = MK::digit(rg);
            e0 = MK::digit(re);
            if constexpr (CLIP) c0 = MK::digit(rc);
        }
        one(col[t * BS], g0, e0 + c0);
        if constexpr (t + 1 < CNT) one(col[(t + 1) * BS], g1, e1 + c1);
        pair_fence();
    });
}
template <class MK, int BS, bool CLIP, bool LEAKY = false>
__device__ __forceinline__ void lds_mult_chunks_k(uint8_t* col, u128 G, u128 E, u128 C, uint32_t ypr,
                                                  LeakyLane lk = LeakyLane{0u, 0u}) {
    static_assert(!(CLIP && LEAKY), "no leaky Clip");
    constexpr int c = static_cast<int>(MK::c), n = static_cast<int>(MK::n), nfull = n / c, tail = n % c;
    // leaky_mult: c ypr + b < Q^2
    const uint32_t yl = LEAKY ? MK::template mod<MK::QQ>(__umul24(lk.fc, ypr) + lk.fb) : 0u;
#pragma unroll 1
    for (int ch = 0; ch < nfull; ++ch) {
        const uint32_t rg = MK::divmod(G), re = MK::divmod(E), rc = CLIP ? MK::divmod(C) : 0u;
        mult_chunk_k<MK, BS, c, CLIP, LEAKY>(col + ch * c * BS, rg, re, rc, ypr, yl, lk.fc);
    }
    if constexpr (tail > 0) {
        const uint32_t rg = MK::divmod(G), re = MK::divmod(E), rc = CLIP ? MK::divmod(C) : 0u;
        mult_chunk_k<MK, BS, tail, CLIP, LEAKY>(col + nfull * c * BS, rg, re, rc, ypr, yl, lk.fc);
    }
}

// Grouped walk: row c < n becomes f(c, row c), G rows per group (load: rows are read; else f gets 0). The
// group's LDS reads are issued together, one exposed latency per group instead of per digit: a digit's
// write-back may alias the next digit's read, so the compiler cannot hoist it.
template <int BS, int G, class F>
__device__ __forceinline__ void lds_group_walk(uint8_t* col, int n, bool load, F&& f) {
    for (int c0 = 0; c0 < n; c0 += G) {
        uint32_t w[G];
#pragma unroll
        for (int u = 0; u < G; ++u) w[u] = (load && c0 + u < n) ? col[(c0 + u) * BS] : 0u;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int c = c0 + u;
            if (c >= n) break;
            col[c * BS] = static_cast<uint8_t>(f(c, w[u]));
        }
    }
}

// ---------------------------------------------------------------------------
// Quad walks: four lanes per (element, residue), lane g of the quad. Power-of-two moduli: a quarter of the
// digits each, g cpl .. g cpl + cpl - 1, which fit one 64-bit window (bits * cpl <= 32 + bits: one 128-bit
// shift per lane instead of one per digit). Odd moduli: the chunks are dealt over the quad, every lane runs
// the chunk divisions and keeps chunk 4 jj + g.

// Rescale: the lane's rows of col (BS-byte rows) become Y = S^-1 L + digits(P) (payload: the digits alone).
// KEY: returns the lane's partial compress(Y) (the quad sums them), else 0.
template <int BS, bool KEY>
__device__ __forceinline__ u128 quad_rescale_walk(uint8_t* col, int n, int g, u128 P, uint32_t inv, bool payload,
                                                  const ModC& m) {
    const uint32_t q = m.q;
    u128 part = 0;
    if (m.bits) {
        const int bb = static_cast<int>(m.bits), cpl = (n + 3) >> 2;
        const uint64_t Pw = static_cast<uint64_t>(P >> (bb * g * cpl));
        for (int t = 0; t < cpl; ++t) {
            const int idx = g * cpl + t;
            if (idx >= n) break;
            const uint32_t pd = static_cast<uint32_t>(Pw >> (bb * t)) & (q - 1);
            const uint32_t v = payload ? pd : modq(static_cast<uint32_t>(col[idx * BS]) * inv + pd, m);
            col[idx * BS] = static_cast<uint8_t>(v);
            if (KEY) part |= static_cast<u128>(v) << (bb * idx);
        }
    } else {
        QPow pw;
        if (KEY) pw.init(m);
        const int c = static_cast<int>(m.c), nch = (n + c - 1) / c;
        u128 Q = P, PW = KEY ? pw.first(g) : static_cast<u128>(0);
        for (int jj = 0; 4 * jj < nch; ++jj) {
            uint32_t mine = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (4 * jj + u >= nch) break;
                const uint32_t r = divmod128(Q, m);
                mine = u == g ? r : mine;
            }
            const int i = 4 * jj + g;
            uint32_t cv = 0, pt = 1;
            for (int t = 0; t < c; ++t) {
                const int idx = i * c + t;
                const uint32_t pd = chunk_digit(mine, m);
                if (idx < n) {
                    const uint32_t v = payload ? pd : modq(static_cast<uint32_t>(col[idx * BS]) * inv + pd, m);  // < p^2 + p
                    col[idx * BS] = static_cast<uint8_t>(v);
                    cv += v * pt;
                }
                pt *= q;
            }
            if (KEY) {
                part += PW * static_cast<u128>(cv);
                PW *= pw.d4;
            }
        }
    }
    return part;
}

// Multiply: the lane's rows of out become E + ypr y - G from the rows y of yc (k_relu_mult's arithmetic).
template <int BS>
__device__ __forceinline__ void quad_mult_walk(const uint8_t* yc, uint8_t* out, int n, int g, u128 G, u128 E,
                                               uint32_t ypr, int p, const ModC& m) {
    const uint32_t q = m.q;
    if (m.bits) {
        const int bb = static_cast<int>(m.bits), cpl = (n + 3) >> 2;
        const uint64_t Gw = static_cast<uint64_t>(G >> (bb * g * cpl)), Ew = static_cast<uint64_t>(E >> (bb * g * cpl));
        for (int t = 0; t < cpl; ++t) {
            const int idx = g * cpl + t;
            if (idx >= n) break;
            const uint32_t gd = static_cast<uint32_t>(Gw >> (bb * t)) & (q - 1);
            const uint32_t ed = static_cast<uint32_t>(Ew >> (bb * t)) & (q - 1);
            out[idx * BS] = static_cast<uint8_t>(mult_digit(ed, ypr, yc[idx * BS], p, gd, m));
        }
    } else {
        const int c = static_cast<int>(m.c), nch = (n + c - 1) / c;
        for (int jj = 0; 4 * jj < nch; ++jj) {
            uint32_t mg = 0, me = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (4 * jj + u >= nch) break;
                const uint32_t rg = divmod128(G, m);
                const uint32_t re = divmod128(E, m);
                mg = u == g ? rg : mg;
                me = u == g ? re : me;
            }
            const int i = 4 * jj + g;
            for (int t = 0; t < c; ++t) {
                const int idx = i * c + t;
                const uint32_t gd = chunk_digit(mg, m);
                const uint32_t ed = chunk_digit(me, m);
                if (idx < n) out[idx * BS] = static_cast<uint8_t>(mult_digit(ed, ypr, yc[idx * BS], p, gd, m));
            }
        }
    }
}

}  // namespace dev
}  // namespace dash
