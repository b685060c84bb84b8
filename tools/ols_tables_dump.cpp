// Writes the raw overlap-save tables of one case (solid_dsp_amd/csrc/ols_tables.cpp) to a file,
// for tests/test_ols_tables.py.  Host only: links ols_tables.cpp and design.cpp, no HIP runtime.
//
//   ols_tables_dump DTYPE LOG2N IN OUT
//
// DTYPE: 0 RR32, 1 RC32, 2 CC32.  LOG2N: 0 for the 4096-point tables, else the long path's log2 N.
// IN: one coefficient (the scale), then the L taps in stored order, raw.  OUT: records of an
// 8-byte name (NUL padded), a uint64 byte count and the data.  The time of the spectrum build
// goes to stderr.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ols_tables.hpp"

using namespace sdsp;

static void put(FILE* f, const char* name, const void* p, size_t bytes) {
    char nm[8] = {};
    std::memcpy(nm, name, std::strlen(name) < 8 ? std::strlen(name) : 8);
    const uint64_t n = bytes;
    std::fwrite(nm, 1, 8, f);
    std::fwrite(&n, 8, 1, f);
    std::fwrite(p, 1, bytes, f);
}
static void put(FILE* f, const char* name, const std::vector<float>& v) { put(f, name, v.data(), v.size() * 4); }

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s DTYPE LOG2N IN OUT\n", argv[0]);
        return 2;
    }
    const int dtype = std::atoi(argv[1]), log2n = std::atoi(argv[2]);
    if (dtype < 0 || dtype > 2 || log2n < 0 || log2n > 22) return 2;
    std::vector<unsigned char> in;
    FILE* fi = std::fopen(argv[3], "rb");
    if (!fi) return 1;
    for (int c; (c = std::fgetc(fi)) != EOF;) in.push_back((unsigned char)c);
    std::fclose(fi);
    const size_t cb = coef_bytes(dtype);
    if (in.size() < 2 * cb || in.size() % cb) return 2;
    const size_t L = in.size() / cb - 1;
    const unsigned char *scale = in.data(), *taps = in.data() + cb;
    FILE* fo = std::fopen(argv[4], "wb");
    if (!fo) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    if (log2n) {
        const std::vector<float> G = ols_long_spectrum(taps, scale, dtype, L, log2n);
        const auto t1 = std::chrono::steady_clock::now();
        put(fo, "lG", G);
        put(fo, "ltw", ols_long_twiddles(log2n));
        // the same spectrum in natural order, restated here: what lG is the [k1][k2] transpose of
        const size_t N = (size_t)1 << log2n;
        std::vector<double> g(2 * N, 0.0);
        const cd s = coef_at(scale, dtype, 0);
        for (size_t i = 0; i < L; ++i) {
            const cd c = coef_at(taps, dtype, L - 1 - i);
            const cd v = coef_is_complex(dtype) ? cmul(c, s) : cd{c.re * s.re, c.re * s.im};
            g[2 * i] = v.re;
            g[2 * i + 1] = v.im;
        }
        host_fft_pow2(g, N);
        std::vector<float> nat(2 * N);
        for (size_t k = 0; k < 2 * N; ++k) nat[k] = (float)(g[k] / (double)N);
        put(fo, "lGnat", nat);
        std::fprintf(stderr, "spectrum %.1f ms\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
    } else {
        const std::vector<cd> G = ols_spectrum(taps, scale, dtype, L);
        const auto t1 = std::chrono::steady_clock::now();
        const std::vector<float> Hs = ols_rows_H(G), tw1 = ols_rows_tw(256, 4096), tw2 = ols_rows_tw(16, 256);
        put(fo, "G", G.data(), G.size() * sizeof(cd));
        put(fo, "Hs", Hs);
        put(fo, "tw1", tw1);
        put(fo, "tw2", tw2);
        put(fo, "pkt", ols_pack_pkt(Hs, tw1, tw2));
        put(fo, "os", ols_os_bases());
        if (ols_real_taps(dtype, scale)) put(fo, "hh", ols_half_table(G));
        std::fprintf(stderr, "spectrum %.1f ms\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    return std::fclose(fo) ? 1 : 0;
}
