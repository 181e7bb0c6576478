// Host-code sanitizer harness for the Gather layer (docs/GATHER.md): garble + host-evaluate + decode the shapes of
// tests/gather_cases.py and the composite circuits (an in_src source, repeats in front of a ReLU, the index labels
// of an ArgMax) on the multi-threaded path. Stand-alone: build it with -fsanitize=address,undefined together with
// core.cpp, gadgets.cpp, garbler.cpp, evaluator.cpp, serialize.cpp and tests/native/gpu_garbler_stub.cpp, and run it
// on the CPU. Exit code 0 = every decoded output equals the expectation computed here from the definition.
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>

#include "layers.h"

using namespace dash;

static int check(const char* name, const std::vector<i64>& got, const std::vector<i64>& want) {
    if (got != want) {
        std::fprintf(stderr, "%s: mismatch\n", name);
        for (size_t i = 0; i < got.size() && i < want.size(); ++i)
            if (got[i] != want[i])
                std::fprintf(stderr, "  %zu: got %lld want %lld\n", i, (long long)got[i], (long long)want[i]);
        return 1;
    }
    std::printf("%s ok\n", name);
    return 0;
}

static LayerSpec gather_spec(const std::vector<i64>& idx, const std::vector<i64>& od, i64 in_src = -2) {
    LayerSpec s;
    s.kind = K_GATHER;
    s.p = {{"idx", idx}, {"od", od}};
    if (in_src != -2) s.p["in_src"] = {in_src};
    return s;
}

static LayerSpec kind_spec(int kind, Params p = {}) {
    LayerSpec s;
    s.kind = kind;
    s.p = std::move(p);
    return s;
}

static std::vector<i64> gather(const std::vector<i64>& x, const std::vector<i64>& idx) {
    std::vector<i64> y(idx.size());
    for (size_t o = 0; o < idx.size(); ++o) y[o] = x[static_cast<size_t>(idx[o])];
    return y;
}

int main() {
    int fails = 0;
    const std::string seed(16, 'a');
    std::mt19937 rng(23);
    const std::vector<int> crt = first_primes(7);
    const std::vector<int> mrs = {102, 7, 7, 6, 6, 6};
    i64 M = 1;
    for (int p : crt) M *= p;
    auto input = [&](i64 n, i64 lim) {
        std::vector<i64> x(n);
        for (auto& v : x) v = static_cast<i64>(rng() % (2 * lim + 1)) - lim;
        return x;
    };
    auto run = [&](const std::vector<LayerSpec>& L, const std::vector<i64>& dims, const std::vector<i64>& x,
                   bool hard) {
        GarbleOptions opt;
        opt.nthreads = 8;
        opt.hardened = hard;
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, dims, opt);
        GarbledModel m2 = GarbledModel::deserialize(m.serialize());  // the model survives its wire form
        return g.decoder().decode(cpu_evaluate(m2, g.encode(x), 8));
    };
    // the plain shapes (Nin, Nout), any signed CRT value, both encodings
    const i64 shapes[7][2] = {{1024, 1024}, {1020, 1020}, {1028, 1028}, {7, 1028}, {2048, 4}, {1023, 1025}, {5, 3}};
    for (const auto& s : shapes) {
        std::vector<i64> idx(s[1]);
        for (auto& v : idx) v = static_cast<i64>(rng() % s[0]);
        idx.front() = s[0] - 1;
        idx.back() = 0;
        std::vector<i64> x = input(s[0], M / 2 - 1);
        x.front() = -(M / 2);
        x.back() = M - M / 2 - 1;
        for (int hard = 0; hard < 2; ++hard) {
            char name[64];
            std::snprintf(name, sizeof(name), "gather(%lld,%lld,%s)", (long long)s[0], (long long)s[1],
                          hard ? "hardened" : "reference");
            fails += check(name, run({gather_spec(idx, {s[1]})}, {s[0]}, x, hard != 0), gather(x, idx));
        }
    }
    {  // repeats in front of a ReLU: one gate per copy
        const std::vector<i64> idx = {0, 0, 1, 4, 4, 4, 2, 3, 3, 0, 1, 4};
        const std::vector<i64> x = {-7, 100000, 0, -200000, 255254};
        std::vector<i64> want = gather(x, idx);
        for (auto& v : want) v = std::max<i64>(v, 0);
        for (int hard = 0; hard < 2; ++hard)
            fails += check(hard ? "gather+relu(hardened)" : "gather+relu(reference)",
                           run({gather_spec(idx, {12}), kind_spec(K_RELU)}, {5}, x, hard != 0), want);
    }
    {  // Conv 1x1 (2 -> 2 on 4 x 4) -> Relu -> Gather(in_src = the conv, a (2, 4, 4) -> (4, 2, 4) view) -> Add(the Relu)
        const std::vector<i64> w = {2, -3, 1, 4}, b = {5, -6};
        const std::vector<i64> x = input(32, 9);
        std::vector<i64> y(32), idx(32);
        for (i64 f = 0; f < 2; ++f)
            for (i64 e = 0; e < 16; ++e) y[f * 16 + e] = b[f] + w[f * 2] * x[e] + w[f * 2 + 1] * x[16 + e];
        std::iota(idx.begin(), idx.end(), 0);
        std::shuffle(idx.begin(), idx.end(), rng);
        std::vector<i64> want = gather(y, idx);
        for (size_t e = 0; e < 32; ++e) want[e] += std::max<i64>(y[e], 0);
        const LayerSpec conv = kind_spec(K_CONV, {{"C", {2}}, {"H", {4}}, {"W", {4}}, {"F", {2}}, {"kh", {1}}, {"kw", {1}},
                                                   {"w", w}, {"b", b}});
        const std::vector<LayerSpec> L = {conv, kind_spec(K_RELU), gather_spec(idx, {2, 4, 4}, 0),
                                          kind_spec(K_ADD, {{"src", {1}}})};
        fails += check("conv+relu+gather(in_src)+add", run(L, {2, 4, 4}, x, true), want);
    }
    {  // ArgMax over 3 candidates at 8 positions, then a Gather of the index labels (hardened only)
        const std::vector<i64> idx = {7, 6, 5, 4, 3, 2, 1, 0, 0, 7, 3, 3};
        const std::vector<i64> x = input(24, 1000);
        std::vector<i64> am(8);
        for (i64 p = 0; p < 8; ++p) {
            i64 best = 0;
            for (i64 c = 1; c < 3; ++c)
                if (x[c * 8 + p] > x[best * 8 + p]) best = c;  // ties go to the lowest index
            am[p] = best;
        }
        const std::vector<LayerSpec> L = {kind_spec(K_ARGMAX, {{"K", {3}}, {"P", {8}}}), gather_spec(idx, {12})};
        fails += check("argmax+gather", run(L, {3, 2, 4}, x, true), gather(am, idx));
    }
    {  // a map that reaches past the input is refused, naming the position
        bool threw = false;
        try {
            run({gather_spec({0, 5}, {2})}, {5}, input(5, 9), true);
        } catch (const std::exception& e) {
            threw = std::string(e.what()).find("position 1") != std::string::npos;
        }
        fails += check("gather(out of range)", {threw ? 1 : 0}, {1});
    }
    return fails ? 1 : 0;
}
