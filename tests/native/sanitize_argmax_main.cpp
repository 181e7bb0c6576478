// Host-code sanitizer harness for the ArgMax layer (docs/ARGMAX.md): garble + host-evaluate + decode ArgMax layers
// over one position (K = 2, 3, 10), over a (5, 7, 11) score map and behind a dense layer, on the multi-threaded
// path. Built with -fsanitize=address,undefined (or thread) by tests/test_argmax_sanitizers.py. Exit code 0 =
// decoded outputs equal the plaintext expectations computed here.
#include <algorithm>
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

// index of the first largest of the K candidates x[c * P + o] of every position o
static std::vector<i64> argmax(const std::vector<i64>& x, i64 K, i64 P) {
    std::vector<i64> r(P, 0);
    for (i64 o = 0; o < P; ++o)
        for (i64 c = 1; c < K; ++c)
            if (x[c * P + o] > x[r[o] * P + o]) r[o] = c;
    return r;
}

int main() {
    int fails = 0;
    const std::string seed(16, 'a');
    std::mt19937 rng(13);
    const std::vector<int> crt = first_primes(7);
    const std::vector<int> mrs = {102, 7, 7, 6, 6, 6};
    GarbleOptions opt;
    opt.nthreads = 8;
    opt.hardened = true;
    const i64 shapes[4][2] = {{2, 1}, {3, 1}, {10, 1}, {5, 77}};
    const char* names[4] = {"argmax(2)", "argmax(3)", "argmax(10)", "argmax(5x7x11)"};
    for (int s = 0; s < 4; ++s) {
        const i64 K = shapes[s][0], P = shapes[s][1];
        std::vector<i64> x(K * P);
        for (auto& v : x) v = static_cast<i64>(rng() % 41) - 20;  // a narrow band: equal maxima happen
        for (i64 c = 0; c < K; ++c) x[c * P] = 7;                 // position 0: all candidates equal
        std::vector<LayerSpec> L(1);
        L[0].kind = K_ARGMAX;
        L[0].p = {{"K", {K}}, {"P", {P}}};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, P == 1 ? std::vector<i64>{K} : std::vector<i64>{K, 7, 11}, opt);
        CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
        fails += check(names[s], g.decoder().decode(out), argmax(x, K, P));
    }
    {  // dense 12 -> 10, ArgMax(10)
        const i64 I = 12, O = 10;
        std::vector<i64> W(I * O), b(O), x(I);
        for (auto& v : W) v = static_cast<i64>(rng() % 9) - 4;
        for (auto& v : b) v = static_cast<i64>(rng() % 11) - 5;
        for (auto& v : x) v = static_cast<i64>(rng() % 41) - 20;
        std::vector<LayerSpec> L(2);
        L[0].kind = K_DENSE;
        L[0].p = {{"in", {I}}, {"out", {O}}, {"w", W}, {"b", b}};
        L[1].kind = K_ARGMAX;
        L[1].p = {{"K", {O}}, {"P", {1}}};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, {I}, opt);
        CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
        std::vector<i64> h(O);
        for (i64 o = 0; o < O; ++o) {
            h[o] = b[o];
            for (i64 i = 0; i < I; ++i) h[o] += W[o * I + i] * x[i];
        }
        fails += check("dense+argmax", g.decoder().decode(out), argmax(h, O, 1));
    }
    return fails ? 1 : 0;
}
