// Host-code sanitizer harness for the dilated Conv2d (docs/DILATED_CONV.md): garble + host-evaluate + decode three
// rows of the suites' shape table (tests/dilated_cases.py), on the multi-threaded path, under both encodings. Built
// with -fsanitize=address,undefined (or thread) by tests/test_dilated_conv_sanitizers.py. Exit code 0 = decoded
// outputs equal the plaintext expectations computed here from the definition.
#include <algorithm>
#include <cstdio>
#include <random>

#include "layers.h"

using namespace dash;

static int check(const std::string& name, const std::vector<i64>& got, const std::vector<i64>& want) {
    if (got != want) {
        std::fprintf(stderr, "%s: mismatch\n", name.c_str());
        for (size_t i = 0; i < got.size() && i < want.size(); ++i)
            if (got[i] != want[i])
                std::fprintf(stderr, "  %zu: got %lld want %lld\n", i, (long long)got[i], (long long)want[i]);
        return 1;
    }
    std::printf("%s ok\n", name.c_str());
    return 0;
}

// the table's order: (W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, groups)
struct Row {
    const char* name;
    i64 W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, g;
};

static LayerSpec conv_spec(const Row& r, const std::vector<i64>& w, const std::vector<i64>& b) {
    LayerSpec s;
    s.kind = K_CONV;
    s.p = {{"C", {r.C}}, {"H", {r.H}}, {"W", {r.W}}, {"F", {r.F}}, {"kh", {r.kh}}, {"kw", {r.kw}}, {"sh", {r.sh}},
           {"sw", {r.sw}}, {"ph", {r.ph}}, {"pw", {r.pw}}, {"w", w}, {"b", b}};
    if (r.g > 1) s.p["g"] = {r.g};
    if (r.dh > 1) s.p["dh"] = {r.dh};
    if (r.dw > 1) s.p["dw"] = {r.dw};
    return s;
}

// the definition, gather form, with the geometry the engines share (ConvGeom: its dh, dw and output size)
static std::vector<i64> conv(const ConvGeom& G, const std::vector<i64>& x, const std::vector<i64>& w,
                             const std::vector<i64>& b) {
    std::vector<i64> y(G.out_size());
    for (i64 f = 0; f < G.F; ++f)
        for (i64 oy = 0; oy < G.OH; ++oy)
            for (i64 ox = 0; ox < G.OW; ++ox) {
                i64 acc = b[f];
                for (i64 c = 0; c < G.Cg(); ++c)
                    for (i64 dy = 0; dy < G.kh; ++dy)
                        for (i64 dx = 0; dx < G.kw; ++dx) {
                            const i64 iy = oy * G.sh - G.ph + dy * G.dh, ix = ox * G.sw - G.pw + dx * G.dw;
                            if (iy < 0 || iy >= G.H || ix < 0 || ix >= G.W) continue;
                            acc += w[((f * G.Cg() + c) * G.kh + dy) * G.kw + dx] *
                                   x[(((f / G.Fg()) * G.Cg() + c) * G.H + iy) * G.W + ix];
                        }
                y[(f * G.OH + oy) * G.OW + ox] = acc;
            }
    return y;
}

int main() {
    int fails = 0;
    const std::string seed(16, 'a');
    std::mt19937 rng(23);
    const std::vector<int> crt = first_primes(7);
    const std::vector<int> mrs;
    const Row rows[3] = {{"d2_same", 7, 6, 4, 5, 3, 3, 1, 1, 2, 2, 2, 2, 1},
                         {"unequal", 9, 8, 5, 3, 3, 2, 2, 1, 1, 0, 1, 3, 1},
                         {"dw_d2", 7, 6, 6, 6, 3, 3, 1, 1, 2, 2, 2, 2, 6}};
    for (const Row& r : rows) {
        std::vector<i64> w(r.F * (r.C / r.g) * r.kh * r.kw), b(r.F), x(r.C * r.H * r.W);
        for (auto& v : w) v = static_cast<i64>(rng() % 13) - 6;
        for (size_t i = 0; i < w.size(); i += 5) w[i] = 0;  // zero and zero-mod-p weights
        for (size_t i = 1; i < w.size(); i += 7) w[i] = 2 * 3 * 5 * 7;
        for (auto& v : b) v = static_cast<i64>(rng() % 19) - 9;
        for (auto& v : x) v = static_cast<i64>(rng() % 41) - 20;
        const LayerSpec spec = conv_spec(r, w, b);
        const ConvGeom G(spec.p);
        if (G.dh != r.dh || G.dw != r.dw || G.OH != (r.H + 2 * r.ph - (r.kh - 1) * r.dh - 1) / r.sh + 1) {
            std::fprintf(stderr, "%s: geometry\n", r.name);
            ++fails;
            continue;
        }
        const std::vector<i64> want = conv(G, x, w, b);
        for (int hard = 0; hard < 2; ++hard) {
            GarbleOptions opt;
            opt.nthreads = 8;
            opt.hardened = hard != 0;
            const std::vector<LayerSpec> L = {spec};
            Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
            GarbledModel m = g.garble(L, {r.C, r.H, r.W}, opt);
            GarbledModel m2 = GarbledModel::deserialize(m.serialize());  // the model survives its wire form
            fails += check(std::string(r.name) + (hard ? "(hardened)" : "(reference)"),
                           g.decoder().decode(cpu_evaluate(m2, g.encode(x), 8)), want);
        }
    }
    return fails ? 1 : 0;
}
