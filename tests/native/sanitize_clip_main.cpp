// Host-code sanitizer harness for the Clip layer (docs/CLIP.md): garble + host-evaluate + decode a Clip and a
// dense -> Clip -> dense circuit, both sign constructions, on the multi-threaded path. Built with
// -fsanitize=address,undefined (or thread) by tests/test_clip_sanitizers.py. Exit code 0 = decoded outputs equal
// the plaintext expectations computed here.
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

int main() {
    int fails = 0;
    const std::string seed(16, 'c');
    std::mt19937 rng(11);
    const std::vector<int> crt = first_primes(7);
    const std::vector<int> mrs = {102, 7, 7, 6, 6, 6};
    for (int exact = 0; exact < 2; ++exact) {
        GarbleOptions opt;
        opt.nthreads = 8;
        opt.hardened = true;
        opt.relu_mrs = exact != 0;
        {  // a single Clip(-37, 41): the values around both bounds, then random ones
            const i64 N = 67, lo = -37, hi = 41;
            std::vector<i64> x(N);
            const i64 edge[6] = {lo - 1, lo, lo + 1, hi - 1, hi, hi + 1};
            for (i64 e = 0; e < N; ++e) x[e] = e < 6 ? edge[e] : static_cast<i64>(rng() % 4001) - 2000;
            std::vector<LayerSpec> L(1);
            L[0].kind = K_CLIP;
            L[0].p = {{"lo", {lo}}, {"hi", {hi}}};
            Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
            GarbledModel m = g.garble(L, {N}, opt);
            CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
            std::vector<i64> want(N);
            for (i64 e = 0; e < N; ++e) want[e] = std::min(std::max(x[e], lo), hi);
            fails += check(exact ? "clip(mrs)" : "clip(approx)", g.decoder().decode(out), want);
        }
        {  // dense 12 -> 9, Clip(-20, 60), dense 9 -> 4
            const i64 I = 12, H = 9, O = 4, lo = -20, hi = 60;
            std::vector<i64> W1(I * H), b1(H), W2(H * O), b2(O), x(I);
            for (auto& v : W1) v = static_cast<i64>(rng() % 9) - 4;
            for (auto& v : b1) v = static_cast<i64>(rng() % 11) - 5;
            for (auto& v : W2) v = static_cast<i64>(rng() % 7) - 3;
            for (auto& v : b2) v = static_cast<i64>(rng() % 11) - 5;
            for (auto& v : x) v = static_cast<i64>(rng() % 41) - 20;
            std::vector<LayerSpec> L(3);
            L[0].kind = K_DENSE;
            L[0].p = {{"in", {I}}, {"out", {H}}, {"w", W1}, {"b", b1}};
            L[1].kind = K_CLIP;
            L[1].p = {{"lo", {lo}}, {"hi", {hi}}};
            L[2].kind = K_DENSE;
            L[2].p = {{"in", {H}}, {"out", {O}}, {"w", W2}, {"b", b2}};
            Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
            GarbledModel m = g.garble(L, {I}, opt);
            CrtLabels out = cpu_evaluate(m, g.encode(x), 8);
            std::vector<i64> h(H), want(O);
            for (i64 o = 0; o < H; ++o) {
                i64 acc = b1[o];
                for (i64 i = 0; i < I; ++i) acc += W1[o * I + i] * x[i];
                h[o] = std::min(std::max(acc, lo), hi);
            }
            for (i64 o = 0; o < O; ++o) {
                want[o] = b2[o];
                for (i64 i = 0; i < H; ++i) want[o] += W2[o * H + i] * h[i];
            }
            fails += check(exact ? "dense+clip(mrs)+dense" : "dense+clip(approx)+dense", g.decoder().decode(out), want);
        }
    }
    return fails ? 1 : 0;
}
