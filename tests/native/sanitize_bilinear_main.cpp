// Host-code sanitizer harness for the Bilinear layer (docs/BILINEAR.md): garble + host-evaluate + decode small
// circuits that hold it, on the multi-threaded path, and the geometry's refusals. Built with
// -fsanitize=address,undefined (or thread) by tests/test_bilinear_sanitizers.py. Exit code 0 = decoded outputs equal
// the plaintext expectations computed here from the definition.
#include <algorithm>
#include <cstdio>
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

// one axis of the half_pixel mode at b fraction bits, in integers: src = ((2 o + 1) n - m) / (2 m), clamped
struct Axis {
    std::vector<i64> i0, i1, n1;
    i64 b;
    Axis(i64 n, i64 m, i64 b_) : b(b_) {
        for (i64 o = 0; o < m; ++o) {
            const i64 den = 2 * m;
            const i64 num = std::min(std::max((2 * o + 1) * n - m, i64(0)), (n - 1) * den);
            const i64 lo = num / den, rem = num % den;
            i0.push_back(lo);
            i1.push_back(std::min(lo + 1, n - 1));
            n1.push_back((2 * rem * (i64(1) << b) + den) / (2 * den));  // floor(lam 2^b + 1/2)
        }
    }
};

static LayerSpec spec(i64 C, i64 H, i64 W, const Axis& y, const Axis& x) {
    LayerSpec s;
    s.kind = K_BILINEAR;
    s.p = {{"C", {C}}, {"H", {H}}, {"W", {W}}, {"OH", {static_cast<i64>(y.i0.size())}},
           {"OW", {static_cast<i64>(x.i0.size())}}, {"by", {y.b}}, {"bx", {x.b}}, {"y0", y.i0}, {"y1", y.i1},
           {"ny", y.n1}, {"x0", x.i0}, {"x1", x.i1}, {"nx", x.n1}};
    return s;
}

// the definition
static std::vector<i64> bilinear(const std::vector<i64>& v, i64 C, i64 H, i64 W, const Axis& y, const Axis& x) {
    const i64 OH = static_cast<i64>(y.i0.size()), OW = static_cast<i64>(x.i0.size());
    std::vector<i64> out(C * OH * OW);
    for (i64 c = 0; c < C; ++c)
        for (i64 oy = 0; oy < OH; ++oy)
            for (i64 ox = 0; ox < OW; ++ox) {
                const i64 wy1 = y.n1[oy], wy0 = (i64(1) << y.b) - wy1, wx1 = x.n1[ox], wx0 = (i64(1) << x.b) - wx1;
                auto at = [&](i64 r, i64 q) { return v[(c * H + r) * W + q]; };
                out[(c * OH + oy) * OW + ox] = wy0 * wx0 * at(y.i0[oy], x.i0[ox]) + wy0 * wx1 * at(y.i0[oy], x.i1[ox]) +
                                               wy1 * wx0 * at(y.i1[oy], x.i0[ox]) + wy1 * wx1 * at(y.i1[oy], x.i1[ox]);
            }
    return out;
}

int main() {
    int fails = 0;
    const std::string seed(16, 'a');
    std::mt19937 rng(17);
    const std::vector<int> mrs;
    auto input = [&](i64 n, int lim) {
        std::vector<i64> x(n);
        for (auto& v : x) v = static_cast<i64>(rng() % (2 * lim + 1)) - lim;
        return x;
    };
    auto run = [&](const std::vector<int>& crt, const std::vector<LayerSpec>& L, const std::vector<i64>& dims,
                   const std::vector<i64>& x) {
        GarbleOptions opt;
        opt.nthreads = 8;
        opt.hardened = true;
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, dims, opt);
        GarbledModel m2 = GarbledModel::deserialize(m.serialize());  // the model survives its wire form
        return g.decoder().decode(cpu_evaluate(m2, g.encode(x), 8));
    };
    {  // factor 2 on both axes: clamped borders, exact weights
        const Axis y(3, 6, 2), x(5, 10, 2);
        const std::vector<i64> v = input(2 * 3 * 5, 20);
        fails += check("bilinear(f2)", run(first_primes(7), {spec(2, 3, 5, y, x)}, {2, 3, 5}, v), bilinear(v, 2, 3, 5, y, x));
    }
    {  // one input row, factor 3 in x at 6 bits (rounded weights)
        const Axis y(1, 2, 0), x(4, 12, 6);
        const std::vector<i64> v = input(3 * 1 * 4, 20);
        fails += check("bilinear(one row, f3)", run(first_primes(7), {spec(3, 1, 4, y, x)}, {3, 1, 4}, v),
                       bilinear(v, 3, 1, 4, y, x));
    }
    {  // two layers in a row on the base (5, 7, 131): weights that vanish mod 5 and 7
        const Axis y(2, 4, 2), x(3, 6, 2), y2(4, 8, 2), x2(6, 6, 0);
        const std::vector<i64> v = input(2 * 2 * 3, 1);
        fails += check("bilinear twice (5, 7, 131)",
                       run({5, 7, 131}, {spec(2, 2, 3, y, x), spec(2, 4, 6, y2, x2)}, {2, 2, 3}, v),
                       bilinear(bilinear(v, 2, 2, 3, y, x), 2, 4, 6, y2, x2));
    }
    {  // the geometry refuses tables that would read or weigh out of range
        const Axis y(3, 6, 2), x(5, 10, 2);
        int refused = 0;
        for (int bad = 0; bad < 4; ++bad) {
            LayerSpec s = spec(2, 3, 5, y, x);
            if (bad == 0) s.p["y1"][5] = 3;
            if (bad == 1) s.p["nx"][2] = 5;
            if (bad == 2) s.p["x0"].pop_back();
            if (bad == 3) s.p["bx"] = {9};
            try {
                BilinearGeom G(s.p);
            } catch (const std::exception&) {
                ++refused;
            }
        }
        fails += check("bilinear refusals", {refused}, {4});
    }
    return fails ? 1 : 0;
}
