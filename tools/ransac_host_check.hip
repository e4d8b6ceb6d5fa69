// Stand-alone host program over csrc/ransac.hpp for a sanitizer build (no GPU, no Python): the draws of K = 3, 4 and 8 at n = K (the last
// step's modulus is 1), K + 1, 8192 and 2^31 - 1 against a plain Fisher-Yates shuffle over a full array, the prefix property of D13's generator,
// the with-replacement rank, the caller's samples -- valid, out of range, negative, repeated -- and the count clamp, on heap buffers of exact size.
//
//   hipcc -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/ransac_host_check.hip -o ransac_host_check
//   ./ransac_host_check           # prints one line per check and "ok"
#include <cstdint>
#include <cstdio>
#include <memory>

#include "../structure-plp-slam_amd/csrc/ransac.hpp"

using namespace plp;

namespace {
constexpr int kBig = 2147483647;                      // 2^31 - 1
const uint64_t kSeeds[4] = {0, 1, 0x123456789ABCDEFull, ~0ull};

struct Args { const int32_t* samples; int iters; unsigned long long seed; };   // what ransac_sample reads of a solver's arguments

// D13 as it is told: shuffle 0 .. n-1 in a full array, step k swaps position k with position k + r_k mod (n - k)
template <int K> void plain_draw(uint64_t seed, int p, int iter, int n, int* out) {
    std::unique_ptr<int[]> a(new int[(size_t)n]);
    for (int i = 0; i < n; ++i) a[i] = i;
    const uint64_t base = mix64(seed ^ mix64(((uint64_t)(uint32_t)p << 32) | (uint64_t)(uint32_t)iter));
    for (int k = 0; k < K; ++k) {
        const uint64_t r = mix64(base + (uint64_t)(k + 1) * 0x9E3779B97F4A7C15ull);
        const int j = k + (int)((uint32_t)(r >> 32) % (uint32_t)(n - k));
        const int t = a[k]; a[k] = a[j]; a[j] = t;
        out[k] = a[k];
    }
}

template <int K> bool check_draws() {
    const int ns[4] = {K, K + 1, 8192, kBig};
    bool good = true;
    int cases = 0;
    for (uint64_t seed : kSeeds)
        for (int p : {0, 7, 65535})
            for (int iter : {0, 1, 1023, kBig})
                for (int n : ns) {
                    std::unique_ptr<int[]> got(new int[K]), want(new int[K]);
                    int idx[K];
                    ransac_draw<K>(seed, p, iter, n, idx);
                    for (int k = 0; k < K; ++k) {
                        got[k] = idx[k];
                        good = good && idx[k] >= 0 && idx[k] < n;
                        for (int l = 0; l < k; ++l) good = good && idx[l] != idx[k];
                    }
                    if (n != kBig) {
                        plain_draw<K>(seed, p, iter, n, want.get());
                        for (int k = 0; k < K; ++k) good = good && got[k] == want[k];
                    }
                    good = good && ransac_draw_one(seed, p, iter, 0, n) == idx[0];   // step 0 moves nothing first: the rank of k = 0 is the first index
                    for (int k = 0; k < 20; ++k) {
                        const int r = ransac_draw_one(seed, p, iter, k, n);
                        good = good && r >= 0 && r < n;
                    }
                    ++cases;
                }
    // the rows of the plp_model_*_draw_host entries and their refusals
    std::unique_ptr<int32_t[]> rows(new int32_t[5 * K]);
    good = good && ransac_draw_rows<K>(42, 3, 10, 5, 257, rows.get()) == 5;
    for (int i = 0; i < 5; ++i) {
        int idx[K];
        ransac_draw<K>(42, 3, 10 + i, 257, idx);
        for (int k = 0; k < K; ++k) good = good && rows[K * i + k] == idx[k];
    }
    good = good && ransac_draw_rows<K>(42, 3, 0, 0, K, nullptr) == 0 && ransac_draw_rows<K>(42, 3, 0, 1, K, nullptr) == -1 &&
           ransac_draw_rows<K>(42, 3, 0, 1, K - 1, rows.get()) == -1 && ransac_draw_rows<K>(42, 3, 0, -1, K, rows.get()) == -1;
    std::printf("ransac_draw<%d>: %d cases: %s\n", K, cases, good ? "ok" : "FAILED");
    return good;
}

// for equal (seed, p, iter, n) the first KA of the KB-draw are the KA-draw: step k depends on the stream and k alone
template <int KA, int KB> bool check_prefix() {
    bool good = true;
    int cases = 0;
    for (uint64_t seed : kSeeds)
        for (int p : {0, 1, 65535})
            for (int iter : {0, 1, 2, 1023})
                for (int n : {8, 9, 64, 257, 8192, kBig}) {
                    int a[KA], b[KB];
                    ransac_draw<KA>(seed, p, iter, n, a);
                    ransac_draw<KB>(seed, p, iter, n, b);
                    for (int k = 0; k < KA; ++k) good = good && a[k] == b[k];
                    ++cases;
                }
    std::printf("prefix %d of %d: %d cases: %s\n", KA, KB, cases, good ? "ok" : "FAILED");
    return good;
}

// the caller's samples of iteration 1 of problem 2 of a P = 3, iters = 2 call: taken as they are, refused when they name no K distinct items
template <int K> bool check_samples() {
    const int P = 3, iters = 2, n = 100;
    std::unique_ptr<int32_t[]> s(new int32_t[(size_t)P * iters * K]);
    for (int i = 0; i < P * iters * K; ++i) s[i] = -7;             // every other row is invalid: a wrong row offset shows
    int32_t* row = s.get() + ((size_t)2 * iters + 1) * K;
    auto fill = [&] { for (int k = 0; k < K; ++k) row[k] = 99 - 2 * k; };
    const Args A{s.get(), iters, 5};
    int idx[K];
    fill();
    bool good = ransac_sample<K>(A, 2, 1, n, idx);
    for (int k = 0; k < K; ++k) good = good && idx[k] == 99 - 2 * k;
    fill(); row[K - 1] = n;                                         // one index equal to n
    good = good && !ransac_sample<K>(A, 2, 1, n, idx);
    fill(); row[0] = -1;                                            // one negative
    good = good && !ransac_sample<K>(A, 2, 1, n, idx);
    fill(); row[K - 1] = row[0];                                    // two equal, the farthest apart ...
    good = good && !ransac_sample<K>(A, 2, 1, n, idx);
    fill(); row[K - 1] = row[K - 2];                                // ... and the last pair
    good = good && !ransac_sample<K>(A, 2, 1, n, idx);
    good = good && !ransac_sample<K>(A, 0, 0, n, idx);              // a row of -7
    const Args D{nullptr, iters, 5};                                // no samples: the draw
    int want[K];
    ransac_draw<K>(5, 2, 1, n, want);
    good = good && ransac_sample<K>(D, 2, 1, n, idx);
    for (int k = 0; k < K; ++k) good = good && idx[k] == want[k];
    std::printf("ransac_sample<%d>: %s\n", K, good ? "ok" : "FAILED");
    return good;
}

bool check_clamp_and_key() {
    std::unique_ptr<int32_t[]> counts(new int32_t[4]{-3, 0, 17, 9000});
    bool good = clamp_count(nullptr, 3, 8192) == 8192 && clamp_count(nullptr, 0, 0) == 0;
    good = good && clamp_count(counts.get(), 0, 8192) == 0 && clamp_count(counts.get(), 1, 8192) == 0 && clamp_count(counts.get(), 2, 8192) == 17 &&
           clamp_count(counts.get(), 3, 8192) == 8192 && clamp_count(counts.get(), 2, 0) == 0 && clamp_count(counts.get(), 0, 0) == 0;
    // more wins; among equals the lowest iteration; the iteration comes back
    good = good && ransac_key(5, 9) > ransac_key(4, 0) && ransac_key(5, 3) > ransac_key(5, 4) && ransac_key(0, 0) > 0ull &&
           ransac_key_iter(ransac_key(0xFFFFFFFFu, 65535)) == 65535 && ransac_key_iter(ransac_key(1, 0)) == 0 && (ransac_key(0x3F800000u, 7) >> 32) == 0x3F800000ull;
    std::printf("clamp_count, ransac_key: %s\n", good ? "ok" : "FAILED");
    return good;
}
}  // namespace

int main() {
    bool good = check_draws<3>();
    good = check_draws<4>() && good;
    good = check_draws<8>() && good;
    good = check_prefix<3, 4>() && good;
    good = check_prefix<4, 8>() && good;
    good = check_samples<3>() && good;
    good = check_samples<4>() && good;
    good = check_samples<8>() && good;
    good = check_clamp_and_key() && good;
    std::printf("%s\n", good ? "ok" : "FAILED");
    return good ? 0 : 1;
}
