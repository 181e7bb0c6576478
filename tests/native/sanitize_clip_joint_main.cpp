// Host-code sanitizer harness for the joint Clip construction (docs/CLIP.md): garble + host-evaluate + decode a
// Rescale(l) + Clip(0, q_hi) pair and a dense -> rescale -> Clip -> dense circuit with GarbleOptions::clip_joint,
// on the multi-threaded path, and a serialize / deserialize round trip of the pair. Built with
// -fsanitize=address,undefined (or thread) by tests/test_clip_joint_sanitizers.py. Exit code 0 = decoded outputs
// equal the plaintext expectations computed here.
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

static i64 ceil_div(i64 x, i64 S) { return x >= 0 ? (x + S - 1) / S : -((-x) / S); }

int main() {
    int fails = 0;
    const std::string seed(16, 'j');
    std::mt19937 rng(13);
    const std::vector<int> crt = first_primes(7);
    const std::vector<int> mrs = {86, 7, 6, 6, 5};
    GarbleOptions opt;
    opt.nthreads = 8;
    opt.hardened = true;
    opt.rescale_mrs = true;
    opt.relu_joint = true;
    opt.clip_joint = true;
    for (const i64 hi : {i64(192), i64(6)}) {  // the pair: values around both thresholds, then random ones
        const i64 N = 131, l = 5, S = i64(1) << l, t_hi = (hi - 1) * S + 1;
        std::vector<i64> x(N);
        const i64 edge[10] = {-S, -S + 1, -S + 2, 0, 1, t_hi - 1, t_hi, t_hi + 1, -255255 + t_hi, 255200};
        for (i64 e = 0; e < N; ++e) x[e] = e < 10 ? edge[e] : static_cast<i64>(rng() % 20001) - 10000;
        std::vector<LayerSpec> L(2);
        L[0].kind = K_RESCALE;
        L[0].p = {{"mode", {0}}, {"l", {l}}};
        L[1].kind = K_CLIP;
        L[1].p = {{"lo", {0}}, {"hi", {hi}}};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, true));
        GarbledModel m = g.garble(L, {N}, opt);
        if (m.layers[1].param("smode", 0) != 2 || m.layers[1].a.count("lo.mrs") || m.layers[1].param("t_hi") != t_hi) {
            std::fprintf(stderr, "pair: the Clip was not garbled with the joint construction\n");
            return 1;
        }
        std::vector<i64> want(N);
        for (i64 e = 0; e < N; ++e) want[e] = std::min(std::max(ceil_div(x[e], S), i64(0)), hi);
        fails += check(hi == 192 ? "rescale+clip(0,192)" : "rescale+clip(0,6)", g.decoder().decode(cpu_evaluate(m, g.encode(x), 8)), want);
        const GarbledModel back = GarbledModel::deserialize(m.serialize());
        fails += check(hi == 192 ? "roundtrip(0,192)" : "roundtrip(0,6)", g.decoder().decode(cpu_evaluate(back, g.encode(x), 8)), want);
    }
    {  // dense 12 -> 9, Rescale(3), Clip(0, 20), dense 9 -> 4
        const i64 I = 12, H = 9, O = 4, l = 3, S = 8, hi = 20;
        std::vector<i64> W1(I * H), b1(H), W2(H * O), b2(O), x(I);
        for (auto& v : W1) v = static_cast<i64>(rng() % 19) - 9;
        for (auto& v : b1) v = static_cast<i64>(rng() % 11) - 5;
        for (auto& v : W2) v = static_cast<i64>(rng() % 7) - 3;
        for (auto& v : b2) v = static_cast<i64>(rng() % 11) - 5;
        for (auto& v : x) v = static_cast<i64>(rng() % 41) - 20;
        std::vector<LayerSpec> L(4);
        L[0].kind = K_DENSE;
        L[0].p = {{"in", {I}}, {"out", {H}}, {"w", W1}, {"b", b1}};
        L[1].kind = K_RESCALE;
        L[1].p = {{"mode", {0}}, {"l", {l}}};
        L[2].kind = K_CLIP;
        L[2].p = {{"lo", {0}}, {"hi", {hi}}};
        L[3].kind = K_DENSE;
        L[3].p = {{"in", {H}}, {"out", {O}}, {"w", W2}, {"b", b2}};
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, true));
        GarbledModel m = g.garble(L, {I}, opt);
        std::vector<i64> h(H), want(O);
        for (i64 o = 0; o < H; ++o) {
            i64 acc = b1[o];
            for (i64 i = 0; i < I; ++i) acc += W1[o * I + i] * x[i];
            h[o] = std::min(std::max(ceil_div(acc, S), i64(0)), hi);
        }
        for (i64 o = 0; o < O; ++o) {
            want[o] = b2[o];
            for (i64 i = 0; i < H; ++i) want[o] += W2[o * H + i] * h[i];
        }
        fails += check("dense+rescale+clip+dense", g.decoder().decode(cpu_evaluate(m, g.encode(x), 8)), want);
    }
    return fails ? 1 : 0;
}
