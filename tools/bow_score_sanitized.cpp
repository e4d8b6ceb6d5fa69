// Stand-alone host run of csrc/bow_score.hpp for a sanitizer build (tests/test_bow_database_cpu.py compiles it with
// -fsanitize=address,undefined and runs it): reads cases from a binary file, scores each in heap arrays of exactly the case's size, and
// prints the f64 bit patterns, then the two f32 threshold expressions for a range of arguments.
//   file: int32 cases; per case int32 na, nb; uint32 wa[na]; double va[na]; uint32 wb[nb]; double vb[nb]
//   usage: bow_score_sanitized CASES.bin
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../structure-plp-slam_amd/csrc/bow_score.hpp"

template <class T> static bool read_n(FILE* f, T* dst, size_t n) { return n == 0 || fread(dst, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t cases = 0;
    if (!read_n(f, &cases, 1) || cases < 0) { fprintf(stderr, "bad header\n"); return 2; }
    for (int32_t c = 0; c < cases; ++c) {
        int32_t n[2];
        if (!read_n(f, n, 2) || n[0] < 0 || n[1] < 0) { fprintf(stderr, "bad case %d\n", c); return 2; }
        // new[] of the exact size, not a vector with spare capacity: a read past the end is a heap overflow the sanitizer sees
        uint32_t* wa = new uint32_t[n[0]]; double* va = new double[n[0]];
        uint32_t* wb = new uint32_t[n[1]]; double* vb = new double[n[1]];
        if (!read_n(f, wa, n[0]) || !read_n(f, va, n[0]) || !read_n(f, wb, n[1]) || !read_n(f, vb, n[1])) { fprintf(stderr, "short case %d\n", c); return 2; }
        const double s = plp::bow_l1_score(wa, va, n[0], wb, vb, n[1]);
        uint64_t bits;
        memcpy(&bits, &s, sizeof bits);
        printf("score %016llx\n", (unsigned long long)bits);
        delete[] wa; delete[] va; delete[] wb; delete[] vb;
    }
    fclose(f);
    for (uint32_t m = 0; m <= 2000; ++m) printf("thr %u %u\n", m, plp::bow_min_common_words(m));
    for (int i = 0; i <= 64; ++i) {
        const float t = plp::bow_min_total_score((float)i / 7.0f);
        uint32_t bits;
        memcpy(&bits, &t, sizeof bits);
        printf("min_total %d %08x\n", i, bits);
    }
    return 0;
}
