// Host-code sanitizer harness for the MatMul layer (docs/MATMUL.md): garble + host-evaluate + decode contractions
// with all four transpose flags and the Gram case on the multi-threaded path, plus matmul_garble_elem /
// matmul_eval_elem called directly on one output element. A stand-alone program with its own main: build it with
// -fsanitize=address,undefined (or thread) together with core.cpp, gadgets.cpp, garbler.cpp, evaluator.cpp,
// serialize.cpp and gpu_garbler_stub.cpp and run it outside pytest. Exit code 0 = decoded outputs equal the
// products computed here.
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
    const i64 M = 13, T = 4, N = 20, lim = 252;  // 4 * 252^2 < M7 / 2
    auto operand = [&]() { return static_cast<i64>(rng() % (2 * lim + 1)) - lim; };
    for (int flags = 0; flags < 4; ++flags) {
        // y = a dense 0 / 1 selection of the input x (reversed, wrapped), the MatMul reads x through in_src
        const bool ta = flags & 1, tb = flags & 2;
        std::vector<i64> x(M * T), W(T * N * M * T, 0), b(T * N, 0), y(T * N);
        for (auto& v : x) v = operand();
        for (i64 t = 0; t < T; ++t) x[ta ? t * M : t] = lim;  // row 0 of x
        for (i64 e = 0; e < T * N; ++e) {
            const i64 src = ((M * T - 1 - e) % (M * T) + M * T) % (M * T);
            W[e * M * T + src] = 1;
            y[e] = x[src];
        }
        std::vector<LayerSpec> L(2);
        L[0].kind = K_DENSE;
        L[0].p = {{"in", {M * T}}, {"out", {T * N}}, {"w", W}, {"b", b}};
        L[1].kind = K_MATMUL;
        L[1].p = {{"src", {0}}, {"M", {M}}, {"T", {T}}, {"N", {N}}, {"in_src", {-1}}};
        if (ta) L[1].p["ta"] = {1};
        if (tb) L[1].p["tb"] = {1};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, {M * T}, opt);
        CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
        std::vector<i64> want(M * N, 0);
        for (i64 i = 0; i < M; ++i)
            for (i64 l = 0; l < N; ++l)
                for (i64 t = 0; t < T; ++t)
                    want[i * N + l] += x[ta ? t * M + i : i * T + t] * y[tb ? l * T + t : t * N + l];
        char name[64];
        std::snprintf(name, sizeof name, "matmul(13, 4, 20) ta=%d tb=%d", int(ta), int(tb));
        fails += check(name, g.decoder().decode(out), want);
    }
    {  // Gram: src = the layer's own input
        const i64 G = 6, K = 5;
        std::vector<i64> x(G * K);
        for (auto& v : x) v = operand() / 2;
        std::vector<LayerSpec> L(1);
        L[0].kind = K_MATMUL;
        L[0].p = {{"src", {-1}}, {"M", {G}}, {"T", {K}}, {"N", {G}}, {"tb", {1}}};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, {G, K}, opt);
        CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
        std::vector<i64> want(G * G, 0);
        for (i64 i = 0; i < G; ++i)
            for (i64 l = 0; l < G; ++l)
                for (i64 t = 0; t < K; ++t) want[i * G + l] += x[i * K + t] * x[l * K + t];
        fails += check("matmul gram(6, 5)", g.decoder().decode(out), want);
    }
    {  // one output element through matmul_garble_elem / matmul_eval_elem: the labels of value sum_t x_t y_t
        const MatMulPlan P(crt, 1, 3, 1, false, false);
        const int k = P.k();
        const i64 xv[3] = {5, -7, 11}, yv[3] = {-3, 2, 9};
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
                lab_axpy(xa[q].data(), pmod(xv[t], mi.p), R.get(mi.p), mi.n, mi.p);
                lab_axpy(ya[q].data(), pmod(yv[t], mi.p), R.get(mi.p), mi.n, mi.p);
                x0p[q] = x0[q].data(), y0p[q] = y0[q].data(), xap[q] = xa[q].data(), yap[q] = ya[q].data();
            }
        for (int j = 0; j < k; ++j) {
            o0[j].resize(mod_info(crt[j]).n), oa[j].resize(mod_info(crt[j]).n);
            o0p[j] = o0[j].data(), oap[j] = oa[j].data();
        }
        std::vector<u128> gt(P.T * P.sum_crt), et(P.T * P.sum_crt);
        matmul_garble_elem(P, R, prg, 3, 0, x0p.data(), y0p.data(), gt.data(), et.data(), o0p.data());
        matmul_eval_elem(P, 3, 0, xap.data(), yap.data(), gt.data(), et.data(), oap.data());
        i64 want = 0;
        for (int t = 0; t < 3; ++t) want += xv[t] * yv[t];
        bool ok = P.entries() == 2 * 58 * 3 && MatMulPlan::entries(crt, 16) == 1856;
        for (int j = 0; j < k && ok; ++j) {
            const ModInfo& mi = mod_info(crt[j]);
            std::vector<comp_t> w = o0[j];
            lab_axpy(w.data(), pmod(want, mi.p), R.get(mi.p), mi.n, mi.p);
            ok = w == oa[j];
        }
        if (!ok) std::fprintf(stderr, "matmul element: mismatch\n");
        else std::printf("matmul element ok\n");
        fails += ok ? 0 : 1;
    }
    return fails ? 1 : 0;
}
