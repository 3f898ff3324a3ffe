// Host build of the window arithmetic of csrc/ordschur.hpp (ord_window with one lane), for
// tests/test_ordschur_window_cpu.py: reads one window and its flags, reorders it, writes the result.
// Compiled as HIP for the host only; needs no device.
//   input : "real" | "cplx", n, then n * n lines "re im" (column-major), then n flags
//   output: swaps, failed, then T (n * n lines "re im"), U likewise, then the n flags
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ordschur.hpp"

using namespace eigsol;

static double& re_of(double& x) { return x; }
static double& re_of(cplx& x) { return x.re; }
static void set_im(double&, double) {}
static void set_im(cplx& x, double v) { x.im = v; }
static double im_of(const double&) { return 0.0; }
static double im_of(const cplx& x) { return x.im; }

template <class S>
static int run(std::ifstream& in, int n, const char* out_path) {
    constexpr int WM = OrdDims<S>::wmax, LD = OrdDims<S>::ld;
    if (n < 1 || n > WM) return 2;
    std::vector<S> t((size_t)WM * LD, s_zero<S>()), u((size_t)WM * LD, s_zero<S>());
    std::vector<unsigned char> f((size_t)n, 0);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            double re, im;
            in >> re >> im;
            re_of(t[i + j * LD]) = re;
            set_im(t[i + j * LD], im);
        }
    for (int i = 0; i < n; ++i) {
        int v;
        in >> v;
        f[i] = v ? 1 : 0;
        re_of(u[i + i * LD]) = 1.0;
    }
    if (!in) return 2;
    int failed = 0;
    const int swaps = dev::ord_window<S>(t.data(), u.data(), f.data(), n, LD, 0, 1, failed);
    FILE* out = std::fopen(out_path, "w");
    if (!out) return 2;
    std::fprintf(out, "%d %d\n", swaps, failed);
    for (const std::vector<S>* m : {&t, &u})
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                S v = (*m)[i + j * LD];
                std::fprintf(out, "%.17g %.17g\n", re_of(v), im_of(v));
            }
    for (int i = 0; i < n; ++i) std::fprintf(out, "%d\n", (int)f[i]);
    std::fclose(out);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    std::string kind;
    int n = 0;
    in >> kind >> n;
    if (!in) return 2;
    return kind == "cplx" ? run<cplx>(in, n, argv[2]) : run<double>(in, n, argv[2]);
}
