// Stand-alone check of native/hbm_pattern.h, built and run by
// tests/test_probe_kernels.py with -fsanitize=address,undefined.  Checks
// that every component of the pattern survives the trip through float
// exactly, at the field boundaries above all, and that no displacement a
// memory fault could produce (a power of two, a multiple of the old
// pattern's 65 536-element period) maps an element onto an equal one.
// Exit 0 = all good.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hbm_pattern.h"

namespace {

int failures = 0;

#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);      \
            ++failures;                    \
        }                                  \
    } while (0)

uint32_t raw(float f) {  // not through the header's bits()
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

bool equal(const hbmpattern::Value &a, const hbmpattern::Value &b) {
    return std::memcmp(&a, &b, sizeof(a)) == 0;
}

// Every field read back from the floats gives i again, and w = x + 0.5.
void check_round_trip(uint64_t i) {
    const hbmpattern::Value v = hbmpattern::value(i);
    const uint64_t x = (uint64_t)v.x, y = (uint64_t)v.y, z = (uint64_t)v.z;
    const unsigned long long ull = i;
    CHECK((float)x == v.x && (float)y == v.y && (float)z == v.z,
          "i=%llu: a component is not an integer", ull);
    CHECK(x < 65536 && y < 65536 && z < 65536, "i=%llu: field too wide", ull);
    CHECK((x | y << 16 | z << 32) == (i & (hbmpattern::kPeriod - 1)),
          "i=%llu: fields do not spell i", ull);
    CHECK((double)v.w == (double)x + 0.5, "i=%llu: w is not x + 0.5", ull);
    CHECK(hbmpattern::matches(i, v.x, v.y, v.z, v.w), "i=%llu: matches(self)", ull);
    CHECK(hbmpattern::bits(v.x) == raw(v.x) && hbmpattern::bits(v.w) == raw(v.w),
          "i=%llu: bits() is not the encoding", ull);
    // one flipped bit in any component is seen, the sign of a zero included
    for (int c = 0; c < 4; ++c)
        for (int bit : {0, 13, 22, 23, 30, 31}) {
            float f[4] = {v.x, v.y, v.z, v.w};
            uint32_t u = raw(f[c]) ^ (1u << bit);
            std::memcpy(&f[c], &u, 4);
            CHECK(!hbmpattern::matches(i, f[0], f[1], f[2], f[3]),
                  "i=%llu: flipped bit %d of component %d passes", ull, bit, c);
        }
}

}  // namespace

int main() {
    const uint64_t P = hbmpattern::kPeriod;
    static_assert(sizeof(hbmpattern::Value) == 16, "one float4");

    // field boundaries
    const uint64_t edges[] = {
        0, 1, 0xFFFE, 0xFFFF, 0x10000, 0x10001, 0x1FFFF, 0x20000,
        0xFFFFFFFEull, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull,
        0xFFFF0000FFFFull, 0xFFFFFFFEFFFFull, P - 2, P - 1};
    for (uint64_t i : edges) check_round_trip(i);

    // the poison is no pattern value: four poison bytes are a negative float
    float poison;
    std::memset(&poison, hbmpattern::kPoisonByte, 4);
    CHECK(poison < 0, "poison float is not negative");
    CHECK(!hbmpattern::matches(0, poison, poison, poison, poison), "poison passes");

    // sampled elements: an LCG over 0..2^48-1 plus the edges
    std::vector<uint64_t> samples(edges, edges + sizeof(edges) / sizeof(edges[0]));
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 4096; ++k) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        samples.push_back(s >> 16);                         // all 48 bits
        if (k % 4 == 0) samples.push_back((s >> 40) << 16);  // x == 0
        if (k % 4 == 1) samples.push_back(s >> 43);          // small, below 2^21
    }
    long pairs = 0;
    for (uint64_t i : samples) {
        check_round_trip(i);
        const hbmpattern::Value v = hbmpattern::value(i);
        for (int k = 0; k < 48; ++k) {
            const uint64_t j = i + ((uint64_t)1 << k);
            if (j >= P) continue;  // injective below 2^48, and no further
            ++pairs;
            CHECK(!equal(v, hbmpattern::value(j)),
                  "pattern(%llu) == pattern(+2^%d)", (unsigned long long)i, k);
            CHECK(!hbmpattern::matches(i, hbmpattern::value(j).x, hbmpattern::value(j).y,
                                       hbmpattern::value(j).z, hbmpattern::value(j).w),
                  "matches(%llu, pattern(+2^%d))", (unsigned long long)i, k);
        }
        for (uint64_t m = 1; m <= 64; ++m) {
            const uint64_t j = i + 65536 * m;
            if (j >= P) continue;
            ++pairs;
            CHECK(!equal(v, hbmpattern::value(j)),
                  "pattern(%llu) == pattern(+65536*%llu)", (unsigned long long)i,
                  (unsigned long long)m);
        }
    }
    // and it does wrap at 2^48: the stated bound is the real one
    CHECK(equal(hbmpattern::value(5), hbmpattern::value(P + 5)), "period is not 2^48");

    if (failures) {
        std::fprintf(stderr, "hbm_pattern_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("hbm_pattern_check: %zu elements, %ld displaced pairs ok\n",
                samples.size(), pairs);
    return 0;
}
