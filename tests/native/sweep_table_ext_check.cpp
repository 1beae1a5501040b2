// Stand-alone check of native/sweep_table_ext.h, built and run by
// tests/test_cu_sweep_ext.py with -fsanitize=address,undefined.  Builds both
// extra tables, then derives each expected result word a second way: it
// reads the element codes back out of the PACKED blob at the offsets the
// kernel uses, decodes them with a decoder of its own (value as a double,
// from sign, exponent and mantissa), takes each lane's true scale from the
// byte its test's select names, places every element at the k that its
// (lane group, element) means to the matrix pipe (written out again here),
// and sums block by block in double, where every partial sum of these
// tables is exact.  Exit 0 = all good.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "sweep_table_ext.h"

namespace {

namespace x = cusweepx;

int failures = 0;

#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);          \
            ++failures;                        \
        }                                      \
    } while (0)

// sign / exponent / mantissa widths and bias, written out again here
struct Layout {
    int bits, E, M, bias;
};
Layout layout(x::Fmt f) {
    switch (f) {
    case x::FP4: return {4, 2, 1, 1};
    case x::FP6: return {6, 2, 3, 1};
    case x::BF6: return {6, 3, 2, 3};
    case x::FP8: return {8, 4, 3, 7};
    case x::BF8: return {8, 5, 2, 15};
    case x::F16: return {16, 5, 10, 15};
    case x::F32: return {32, 8, 23, 127};
    case x::F64: return {64, 11, 52, 1023};
    case x::I8: return {8, 0, 0, 0};
    }
    std::abort();
}

double decode(x::Fmt f, uint64_t code) {
    const Layout l = layout(f);
    if (f == x::I8) return (double)(int8_t)(uint8_t)code;
    const double sign = code >> (l.bits - 1) & 1 ? -1.0 : 1.0;
    const int e = (int)(code >> l.M & ((1ull << l.E) - 1));
    const double m = (double)(code & ((1ull << l.M) - 1)) / (double)(1ull << l.M);
    return e ? sign * std::ldexp(1.0 + m, e - l.bias) : sign * std::ldexp(m, 1 - l.bias);
}

// element j of the fragment at `frag`, nbits wide, from a little-endian
// bit string; reads only the bytes that hold it
uint64_t element(const uint8_t *frag, int j, int nbits) {
    uint64_t code = 0;
    for (int b = 0; b < nbits; ++b) {
        const int pos = j * nbits + b;
        code |= (uint64_t)(frag[pos / 8] >> (pos % 8) & 1) << b;
    }
    return code;
}

uint32_t word_at(const uint8_t *p) {
    uint32_t w;
    std::memcpy(&w, p, 4);
    return w;
}

void check_test(int set, int p, int t, const std::vector<uint8_t> &blob) {
    const x::PipeDesc &d = x::desc(set, p);
    const x::TestVector v = x::make_test(set, p, t);
    const int J = x::ext_lane_elems(set, p), groups = x::kLanes / d.M;
    const int fa = x::frag_bytes(set, p, 0), fb = x::frag_bytes(set, p, 1);
    const int regs = x::regs(set, p), results = x::ext_results(set, p);
    const bool scaled = x::scaled(set);

    CHECK(J * groups == d.K, "%s: slots", d.name);
    CHECK(results * x::kLanes == d.M * d.N, "%s: results", d.name);
    CHECK(!scaled || J == 32, "%s: one lane is one MX block", d.name);
    CHECK(x::test_offset(set, p, t) + x::test_bytes(set, p) <= (int)blob.size(),
          "%s t%d: past the blob", d.name, t);
    CHECK(v.abs_sum_max < x::exact_bound(d.result), "%s t%d: bound", d.name, t);

    const uint8_t *a_at = blob.data() + x::test_offset(set, p, t);
    const uint8_t *b_at = a_at + x::kLanes * fa;
    const uint8_t *sa_at = b_at + x::kLanes * fb;
    const uint8_t *sb_at = sa_at + 4 * x::kLanes;
    const uint8_t *want_at = scaled ? sb_at + 4 * x::kLanes : sa_at;
    CHECK(std::memcmp(a_at, v.a_frag.data(), v.a_frag.size()) == 0, "%s: blob A", d.name);
    CHECK(std::memcmp(b_at, v.b_frag.data(), v.b_frag.size()) == 0, "%s: blob B", d.name);

    // the block scale of (row or column rc, group g) as the hardware picks
    // it: that lane's word, the byte the test's select names
    auto scale = [&](const uint8_t *at, int sel, int rc, int g) {
        if (!scaled) return 0;
        const uint32_t w = word_at(at + 4 * (g * d.M + rc));
        return (int)(w >> (8 * sel) & 0xFF) - 127;
    };
    if (scaled)
        for (int l = 0; l < x::kLanes; ++l)
            for (int side = 0; side < 2; ++side) {
                const uint32_t w = word_at((side ? sb_at : sa_at) + 4 * l);
                const int sel = side ? x::sel_b(t) : x::sel_a(t);
                const int truth = (int)(w >> (8 * sel) & 0xFF);
                for (int k = 0; k < 4; ++k)
                    CHECK(k == sel || std::abs((int)(w >> (8 * k) & 0xFF) - truth) >= 8,
                          "%s t%d lane %d: decoy too near", d.name, t, l);
            }

    // A [M][K] and B [K][N] by k: element e of lane group g is k = g J + e,
    // except on the 8-bit side of fp8 x fp4, whose lanes hold two halves
    auto k_of = [&](x::Fmt f, int g, int e) {
        const bool halves = scaled && d.a != d.b && layout(f).bits == 8;
        return !halves ? g * J + e : e < 16 ? 16 * g + e : 64 + 16 * g + (e - 16);
    };
    std::vector<double> A((size_t)d.M * d.K, NAN), B((size_t)d.K * d.N, NAN);
    for (int l = 0; l < x::kLanes; ++l)
        for (int e = 0; e < J; ++e) {
            A[(size_t)(l % d.M) * d.K + k_of(d.a, l / d.M, e)] =
                decode(d.a, element(a_at + (size_t)l * fa, e, layout(d.a).bits));
            B[(size_t)k_of(d.b, l / d.M, e) * d.N + l % d.N] =
                decode(d.b, element(b_at + (size_t)l * fb, e, layout(d.b).bits));
        }
    for (double v0 : A) CHECK(!std::isnan(v0), "%s: A not covered", d.name);
    for (double v0 : B) CHECK(!std::isnan(v0), "%s: B not covered", d.name);

    // the scale of lane group g belongs to the k-block g of its row / column
    std::vector<double> D((size_t)d.M * d.N);
    for (int i = 0; i < d.M; ++i)
        for (int j = 0; j < d.N; ++j) {
            double sum = 0;
            for (int g = 0; g < groups; ++g) {
                const int e = scale(sa_at, x::sel_a(t), i, g) + scale(sb_at, x::sel_b(t), j, g);
                for (int k = g * J; k < (g + 1) * J; ++k)
                    sum += std::ldexp(A[(size_t)i * d.K + k] * B[(size_t)k * d.N + j], e);
            }
            D[(size_t)i * d.N + j] = sum;
            CHECK(sum == std::ldexp((double)v.D[(size_t)i * d.N + j], -v.unit_shift),
                  "%s t%d (%d, %d): D", d.name, t, i, j);
        }

    // rows pairwise distinct, columns pairwise distinct, D != D^T
    std::set<std::vector<double>> rows, cols;
    bool symmetric = true;
    for (int i = 0; i < d.M; ++i) {
        std::vector<double> row, col;
        for (int j = 0; j < d.N; ++j) {
            row.push_back(D[(size_t)i * d.N + j]);
            col.push_back(D[(size_t)j * d.N + i]);
            if (row.back() != col.back()) symmetric = false;
        }
        rows.insert(row);
        cols.insert(col);
    }
    CHECK((int)rows.size() == d.M, "%s t%d: repeated row", d.name, t);
    CHECK((int)cols.size() == d.N, "%s t%d: repeated column", d.name, t);
    CHECK(!symmetric, "%s t%d: D == D^T", d.name, t);

    for (int l = 0; l < x::kLanes; ++l)
        for (int r = 0; r < results; ++r) {
            const int row = d.result == x::RF64 ? (l >> 4) + 4 * r
                            : d.M == 16         ? 4 * (l >> 4) + r
                                                : (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            CHECK(row == x::ext_result_row(set, p, l, r), "%s: row map", d.name);
            const double val = D[(size_t)row * d.N + l % d.N];
            uint32_t words[2] = {0, 0};
            int n = 1;
            if (d.result == x::RI32) {
                words[0] = (uint32_t)(int32_t)val;
            } else if (d.result == x::RF32) {
                const float f = (float)val;
                CHECK((double)f == val, "%s t%d: not exact in f32", d.name, t);
                std::memcpy(words, &f, 4);
            } else {
                std::memcpy(words, &val, 8);
                n = 2;
            }
            for (int k = 0; k < n; ++k)
                CHECK(words[k] == word_at(want_at + 4 * ((size_t)l * regs + (size_t)r * n + k)),
                      "%s t%d lane %d result %d: expected word", d.name, t, l, r);
        }
}

}  // namespace

int main() {
    for (int set : {(int)x::kMx, (int)x::kWide}) {
        const std::vector<uint8_t> blob = x::build_table(set);
        CHECK((int)blob.size() == x::table_bytes(set), "blob size");
        CHECK(x::lds_bytes(set) >= x::table_bytes(set) && x::lds_bytes(set) > 80 * 1024,
              "lds bytes");
        for (int p = 0; p < x::n_pipes(set); ++p)
            for (int t = 0; t < x::kTests; ++t) check_test(set, p, t, blob);
    }
    CHECK(x::build_table(x::kBase) == cusweep::build_table(), "base table");
    if (failures) {
        std::fprintf(stderr, "sweep_table_ext_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("sweep_table_ext_check: %d + %d pipes x %d tests ok, %d + %d table bytes\n",
                x::kMxPipes, x::kWidePipes, x::kTests, x::table_bytes(x::kMx),
                x::table_bytes(x::kWide));
    return 0;
}
