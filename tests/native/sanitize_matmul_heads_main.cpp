// Host-code sanitizer harness for the multi-head MatMul layer (docs/MATMUL.md, Heads): garble + host-evaluate +
// decode G = 3 contractions with all four transpose flags and the Gram case on the multi-threaded path, plus
// matmul_garble_elem / matmul_eval_elem called directly on an output element of the last head, its operands picked
// by MatMulPlan::xidx / yidx. A stand-alone program with its own main: build it with -fsanitize=address,undefined
// (or thread) together with core.cpp, gadgets.cpp, garbler.cpp, evaluator.cpp, serialize.cpp and
// gpu_garbler_stub.cpp and run it outside pytest. Exit code 0 = decoded outputs equal the products computed here.
#include <cstdio>
#include <random>

#include "model.h"

using namespace dash;

static int check(const char* name, const std::vector<i64>& got, const std::vector<i64>& want) {
    if (got != want) {
        std::fprintf(stderr, "%s: mismatch\n", name);
        for (size_t i = 0; i < got.size() && i < want.size(); ++i)
            std::fprintf(stderr, "  %zu: got %lld want %lld\n", i, (long long)got[i], (long long)want[i]);
        return 1;
    }
    std::printf("%s ok\n", name);
    return 0;
}

int main() {
    int fails = 0;
    const std::string seed(16, 'a');
    std::mt19937 rng(17);
    const std::vector<int> crt = first_primes(7);
    const std::vector<int> mrs = {102, 7, 7, 6, 6, 6};
    GarbleOptions opt;
    opt.nthreads = 8;
    opt.hardened = true;
    const i64 G = 3, M = 5, T = 4, N = 7, lim = 252;  // 4 * 252^2 < M7 / 2
    const i64 nx = G * M * T, ny = G * T * N;
    auto operand = [&]() { return static_cast<i64>(rng() % (2 * lim + 1)) - lim; };
    for (int flags = 0; flags < 4; ++flags) {
        // y = a dense 0 / 1 selection of the input x (reversed, wrapped), the MatMul reads x through in_src
        const bool ta = flags & 1, tb = flags & 2;
        std::vector<i64> x(nx), W(ny * nx, 0), b(ny, 0), y(ny);
        for (auto& v : x) v = operand();
        for (i64 g = 0; g < G; ++g)
            for (i64 t = 0; t < T; ++t) x[g * M * T + (ta ? t * M : t)] = lim;  // row 0 of every head of x
        for (i64 e = 0; e < ny; ++e) {
            const i64 src = ((nx - 1 - e) % nx + nx) % nx;
            W[e * nx + src] = 1;
            y[e] = x[src];
        }
        std::vector<LayerSpec> L(2);
        L[0].kind = K_DENSE;
        L[0].p = {{"in", {nx}}, {"out", {ny}}, {"w", W}, {"b", b}};
        L[1].kind = K_MATMUL;
        L[1].p = {{"src", {0}}, {"M", {M}}, {"T", {T}}, {"N", {N}}, {"G", {G}}, {"in_src", {-1}}};
        if (ta) L[1].p["ta"] = {1};
        if (tb) L[1].p["tb"] = {1};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, {nx}, opt);
        CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
        std::vector<i64> want(G * M * N, 0);
        for (i64 h = 0; h < G; ++h)
            for (i64 i = 0; i < M; ++i)
                for (i64 l = 0; l < N; ++l)
                    for (i64 t = 0; t < T; ++t)
                        want[(h * M + i) * N + l] += x[h * M * T + (ta ? t * M + i : i * T + t)] *
                                                     y[h * T * N + (tb ? l * T + t : t * N + l)];
        char name[64];
        std::snprintf(name, sizeof name, "matmul heads(3, 5, 4, 7) ta=%d tb=%d", int(ta), int(tb));
        fails += check(name, g.decoder().decode(out), want);
    }
    {  // Gram per head: src = the layer's own input
        const i64 R = 4, K = 5;
        std::vector<i64> x(G * R * K);
        for (auto& v : x) v = operand() / 2;
        std::vector<LayerSpec> L(1);
        L[0].kind = K_MATMUL;
        L[0].p = {{"src", {-1}}, {"M", {R}}, {"T", {K}}, {"N", {R}}, {"G", {G}}, {"tb", {1}}};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, {G * R, K}, opt);
        CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
        std::vector<i64> want(G * R * R, 0);
        for (i64 h = 0; h < G; ++h)
            for (i64 i = 0; i < R; ++i)
                for (i64 l = 0; l < R; ++l)
                    for (i64 t = 0; t < K; ++t)
                        want[(h * R + i) * R + l] += x[(h * R + i) * K + t] * x[(h * R + l) * K + t];
        fails += check("matmul heads gram(3, 4, 5)", g.decoder().decode(out), want);
    }
    {  // the last output of the last head through matmul_garble_elem / matmul_eval_elem, operands by xidx / yidx
        const MatMulPlan P(crt, 2, 3, 2, true, false, 2);  // G = 2 heads of (M, T, N) = (2, 3, 2), x stored T x M
        const int k = P.k();
        const i64 o = P.nout() - 1;  // head 1, i = 1, l = 1
        const i64 xv[12] = {5, -7, 11, 2, -3, 4, 6, -1, 8, -9, 10, 3}, yv[12] = {-3, 2, 9, 1, -5, 7, 4, -2, 6, -8, 12, -4};
        bool ok = P.nx() == 12 && P.ny() == 12 && P.nout() == 8;
        i64 want = 0;
        for (i64 t = 0; t < 3; ++t) {
            // head 1's slabs start at element 6; x_1[i, t] = slab[t M + i], y_1[t, l] = slab[t N + l]
            ok = ok && P.xidx(o, t) == 6 + t * 2 + 1 && P.yidx(o, t) == 6 + t * 2 + 1;
            want += xv[P.xidx(o, t)] * yv[P.yidx(o, t)];
        }
        std::vector<LayerSpec> L(1);
        L[0].kind = K_FLATTEN;
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        g.garble(L, {1}, opt);  // garbling draws the offset labels
        const LabelBank& R = g.offsets();
        const Prg prg;  // any PRG: the gates only need fresh-looking draws
        std::vector<std::vector<comp_t>> x0(3 * k), y0(3 * k), xa(3 * k), ya(3 * k), o0(k), oa(k);
        std::vector<const comp_t*> x0p(3 * k), y0p(3 * k), xap(3 * k), yap(3 * k);
        std::vector<comp_t*> o0p(k), oap(k);
        u64 ctr = 0;
        for (int t = 0; t < 3; ++t)
            for (int j = 0; j < k; ++j) {
                const ModInfo& mi = mod_info(crt[j]);
                const int q = t * k + j;
                x0[q].resize(mi.n), y0[q].resize(mi.n);
                prg.label(stream_id(kGlobalLayer, 7, q), ctr, mi.p, mi.n, x0[q].data());
                prg.label(stream_id(kGlobalLayer, 8, q), ctr, mi.p, mi.n, y0[q].data());
                xa[q] = x0[q], ya[q] = y0[q];
                lab_axpy(xa[q].data(), pmod(xv[P.xidx(o, t)], mi.p), R.get(mi.p), mi.n, mi.p);
                lab_axpy(ya[q].data(), pmod(yv[P.yidx(o, t)], mi.p), R.get(mi.p), mi.n, mi.p);
                x0p[q] = x0[q].data(), y0p[q] = y0[q].data(), xap[q] = xa[q].data(), yap[q] = ya[q].data();
            }
        for (int j = 0; j < k; ++j) {
            o0[j].resize(mod_info(crt[j]).n), oa[j].resize(mod_info(crt[j]).n);
            o0p[j] = o0[j].data(), oap[j] = oa[j].data();
        }
        std::vector<u128> gt(P.T * P.sum_crt), et(P.T * P.sum_crt);
        matmul_garble_elem(P, R, prg, 3, o, x0p.data(), y0p.data(), gt.data(), et.data(), o0p.data());
        matmul_eval_elem(P, 3, o, xap.data(), yap.data(), gt.data(), et.data(), oap.data());
        ok = ok && P.entries() == 2 * 58 * 3;
        for (int j = 0; j < k && ok; ++j) {
            const ModInfo& mi = mod_info(crt[j]);
            std::vector<comp_t> w = o0[j];
            lab_axpy(w.data(), pmod(want, mi.p), R.get(mi.p), mi.n, mi.p);
            ok = w == oa[j];
        }
        if (!ok) std::fprintf(stderr, "matmul heads element: mismatch\n");
        else std::printf("matmul heads element ok\n");
        fails += ok ? 0 : 1;
    }
    return fails ? 1 : 0;
}
