// Host-code sanitizer harness for the ConvTranspose2d and Upsample layers (docs/CONV_TRANSPOSE.md): garble +
// host-evaluate + decode small circuits that hold both, on the multi-threaded path. Built with
// -fsanitize=address,undefined (or thread) by tests/test_conv_transpose_sanitizers.py. Exit code 0 = decoded
// outputs equal the plaintext expectations computed here from the definition.
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

struct CT {
    i64 C, H, W, F, kh, kw, sh, sw, ph, pw, oph, opw;
    i64 OH() const { return (H - 1) * sh - 2 * ph + kh + oph; }
    i64 OW() const { return (W - 1) * sw - 2 * pw + kw + opw; }
};

// the definition, scatter form: every input pixel adds its weighted kernel to the output
static std::vector<i64> convt(const CT& g, const std::vector<i64>& x, const std::vector<i64>& w,
                              const std::vector<i64>& b) {
    const i64 OH = g.OH(), OW = g.OW();
    std::vector<i64> y(g.F * OH * OW);
    for (i64 f = 0; f < g.F; ++f)
        for (i64 o = 0; o < OH * OW; ++o) y[f * OH * OW + o] = b[f];
    for (i64 c = 0; c < g.C; ++c)
        for (i64 iy = 0; iy < g.H; ++iy)
            for (i64 ix = 0; ix < g.W; ++ix)
                for (i64 f = 0; f < g.F; ++f)
                    for (i64 dy = 0; dy < g.kh; ++dy)
                        for (i64 dx = 0; dx < g.kw; ++dx) {
                            const i64 oy = iy * g.sh + dy - g.ph, ox = ix * g.sw + dx - g.pw;
                            if (oy < 0 || oy >= OH || ox < 0 || ox >= OW) continue;
                            y[(f * OH + oy) * OW + ox] +=
                                w[((c * g.F + f) * g.kh + dy) * g.kw + dx] * x[(c * g.H + iy) * g.W + ix];
                        }
    return y;
}

static std::vector<i64> upsample(const std::vector<i64>& x, i64 C, i64 H, i64 W, i64 fh, i64 fw) {
    std::vector<i64> y(C * H * fh * W * fw);
    for (i64 c = 0; c < C; ++c)
        for (i64 oy = 0; oy < H * fh; ++oy)
            for (i64 ox = 0; ox < W * fw; ++ox)
                y[(c * H * fh + oy) * W * fw + ox] = x[(c * H + oy / fh) * W + ox / fw];
    return y;
}

static LayerSpec convt_spec(const CT& g, const std::vector<i64>& w, const std::vector<i64>& b) {
    LayerSpec s;
    s.kind = K_CONVT;
    s.p = {{"C", {g.C}}, {"H", {g.H}}, {"W", {g.W}}, {"F", {g.F}}, {"kh", {g.kh}}, {"kw", {g.kw}}, {"sh", {g.sh}},
           {"sw", {g.sw}}, {"ph", {g.ph}}, {"pw", {g.pw}}, {"oph", {g.oph}}, {"opw", {g.opw}}, {"w", w}, {"b", b}};
    return s;
}

static LayerSpec up_spec(i64 C, i64 H, i64 W, i64 fh, i64 fw) {
    LayerSpec s;
    s.kind = K_UPSAMPLE;
    s.p = {{"C", {C}}, {"H", {H}}, {"W", {W}}, {"fh", {fh}}, {"fw", {fw}}};
    return s;
}

int main() {
    int fails = 0;
    const std::string seed(16, 'a');
    std::mt19937 rng(17);
    const std::vector<int> crt = first_primes(7);
    const std::vector<int> mrs;
    auto weights = [&](const CT& g, std::vector<i64>& w, std::vector<i64>& b) {
        w.resize(g.C * g.F * g.kh * g.kw);
        b.resize(g.F);
        for (auto& v : w) v = static_cast<i64>(rng() % 13) - 6;
        for (size_t i = 0; i < w.size(); i += 5) w[i] = 0;  // zero and zero-mod-p weights
        for (size_t i = 1; i < w.size(); i += 7) w[i] = 2 * 3 * 5 * 7;
        for (auto& v : b) v = static_cast<i64>(rng() % 19) - 9;
    };
    auto input = [&](i64 n) {
        std::vector<i64> x(n);
        for (auto& v : x) v = static_cast<i64>(rng() % 41) - 20;
        return x;
    };
    auto run = [&](const std::vector<LayerSpec>& L, const std::vector<i64>& dims, const std::vector<i64>& x,
                   bool hard) {
        GarbleOptions opt;
        opt.nthreads = 8;
        opt.hardened = hard;
        Garbler g(crt, mrs, seed, required_max_modulus(crt, mrs, L, false));
        GarbledModel m = g.garble(L, dims, opt);
        // the model survives its wire form
        GarbledModel m2 = GarbledModel::deserialize(m.serialize());
        return g.decoder().decode(cpu_evaluate(m2, g.encode(x), 8));
    };
    const CT shapes[3] = {{3, 4, 5, 4, 3, 3, 2, 2, 1, 1, 1, 1},   // k3 s2 p1 op1
                          {2, 3, 4, 3, 4, 4, 2, 2, 1, 1, 0, 0},   // k4 s2 p1
                          {2, 4, 3, 2, 3, 2, 1, 2, 0, 1, 0, 0}};  // non-square kernel, unequal strides
    const char* names[3] = {"convt(k3s2p1op1)", "convt(k4s2p1)", "convt(unequal)"};
    for (int s = 0; s < 3; ++s) {
        const CT& g = shapes[s];
        std::vector<i64> w, b;
        weights(g, w, b);
        const std::vector<i64> x = input(g.C * g.H * g.W);
        fails += check(names[s], run({convt_spec(g, w, b)}, {g.C, g.H, g.W}, x, true), convt(g, x, w, b));
    }
    {  // Upsample(2, 3) -> ConvTranspose2d -> Upsample(2, 1)
        const CT g{2, 4, 9, 3, 2, 2, 2, 2, 0, 0, 0, 0};
        std::vector<i64> w, b;
        weights(g, w, b);
        const std::vector<i64> x = input(2 * 2 * 3);
        const std::vector<LayerSpec> L = {up_spec(2, 2, 3, 2, 3), convt_spec(g, w, b), up_spec(3, g.OH(), g.OW(), 2, 1)};
        const std::vector<i64> want =
            upsample(convt(g, upsample(x, 2, 2, 3, 2, 3), w, b), 3, g.OH(), g.OW(), 2, 1);
        fails += check("up+convt+up", run(L, {2, 2, 3}, x, true), want);
    }
    {  // Upsample alone under the reference encoding
        const std::vector<i64> x = input(3 * 2 * 5);
        fails += check("upsample(reference)", run({up_spec(3, 2, 5, 3, 2)}, {3, 2, 5}, x, false),
                       upsample(x, 3, 2, 5, 3, 2));
    }
    return fails ? 1 : 0;
}
