// Host-code sanitizer harness for the Mul layer (docs/MUL.md): garble + host-evaluate + decode an elementwise
// product, a channel broadcast and a square on the multi-threaded path, plus mul_garble_elem / mul_eval_elem called
// directly on one element. A stand-alone program with its own main: build it with -fsanitize=address,undefined (or
// thread) together with core.cpp, gadgets.cpp, garbler.cpp, evaluator.cpp, serialize.cpp and gpu_garbler_stub.cpp
// and run it outside pytest. Exit code 0 = decoded outputs equal the products computed here.
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
    auto operand = [&]() { return static_cast<i64>(rng() % 1011) - 505; };  // 505^2 < M / 2
    {  // elementwise: y = the circuit input (src = -1), x = the input behind a flatten
        const i64 N = 77;
        std::vector<i64> x(N);
        for (auto& v : x) v = operand();
        x[0] = 505, x[N - 1] = -505;
        std::vector<LayerSpec> L(2);
        L[0].kind = K_FLATTEN;
        L[1].kind = K_MUL;
        L[1].p = {{"src", {-1}}};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, {N}, opt);
        CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
        std::vector<i64> want(N);
        for (i64 e = 0; e < N; ++e) want[e] = x[e] * x[e];
        fails += check("mul(77) src=-1", g.decoder().decode(out), want);
    }
    {  // broadcast: a dense layer picks one element per channel as y, the Mul reads the input through in_src
        const i64 C = 3, bc = 20, N = C * bc;
        std::vector<i64> x(N), W(C * N, 0), b(C, 0);
        for (auto& v : x) v = operand();
        for (i64 c = 0; c < C; ++c) W[c * N + c * bc + 1] = 1;
        std::vector<LayerSpec> L(2);
        L[0].kind = K_DENSE;
        L[0].p = {{"in", {N}}, {"out", {C}}, {"w", W}, {"b", b}};
        L[1].kind = K_MUL;
        L[1].p = {{"src", {0}}, {"bc", {bc}}, {"in_src", {-1}}};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, {C, 4, 5}, opt);
        CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
        std::vector<i64> want(N);
        for (i64 e = 0; e < N; ++e) want[e] = x[e] * x[(e / bc) * bc + 1];
        fails += check("mul(3x4x5) bc=20", g.decoder().decode(out), want);
    }
    {  // square
        const i64 N = 272;
        std::vector<i64> x(N);
        for (auto& v : x) v = operand();
        std::vector<LayerSpec> L(1);
        L[0].kind = K_MUL;
        L[0].p = {{"sq", {1}}};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, {N}, opt);
        CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
        std::vector<i64> want(N);
        for (i64 e = 0; e < N; ++e) want[e] = x[e] * x[e];
        fails += check("mul.square(272)", g.decoder().decode(out), want);
    }
    {  // MulPlan's sizes
        const MulPlan prod(crt, 0, false), sq(crt, 0, true), bcp(crt, 20, false);
        const bool ok = prod.entries() == 116 && sq.entries() == 58 && MulPlan::entries(crt, true) == 58 &&
                        bcp.ysrc(59) == 2 && bcp.ny(60) == 3 && prod.ysrc(59) == 59 && prod.ny(60) == 60;
        if (!ok) std::fprintf(stderr, "MulPlan sizes: mismatch\n");
        else std::printf("MulPlan sizes ok\n");
        fails += ok ? 0 : 1;
    }
    return fails ? 1 : 0;
}
