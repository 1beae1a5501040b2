// Stand-alone check of native/sweep_table.h, built and run by
// tests/test_cu_sweep.py with -fsanitize=address,undefined.  Builds every
// table, then derives each expected result a second way: it decodes the
// PACKED per-lane fragments and pairs element j of lane group h in A with
// the same (h, j) in B, as the matrix pipe does.  Exit 0 = all good.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "sweep_table.h"

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

int decode(cusweep::Elem e, const uint8_t *src) {
    if (e == cusweep::BF16 || e == cusweep::F16) {
        uint16_t bits;
        std::memcpy(&bits, src, 2);
        const uint16_t *tab = e == cusweep::BF16 ? cusweep::kBf16Bits : cusweep::kF16Bits;
        for (int i = 0; i < 5; ++i)
            if (tab[i] == bits) return i - 2;
    } else {
        const uint8_t *tab = e == cusweep::FP8 ? cusweep::kFp8Bits : cusweep::kI8Bits;
        for (int i = 0; i < 5; ++i)
            if (tab[i] == *src) return i - 2;
    }
    std::fprintf(stderr, "undecodable operand\n");
    std::exit(1);
}

void check_test(int p, int t, const std::vector<uint8_t> &blob) {
    const cusweep::PipeDesc &d = cusweep::kPipeDesc[p];
    const cusweep::TestVector v = cusweep::make_test(p, t);
    const int J = cusweep::lane_elems(p), eb = cusweep::elem_bytes(d.elem);
    const int fb = cusweep::frag_bytes(p), groups = cusweep::kLanes / d.M;

    CHECK(d.regs * cusweep::kLanes == d.M * d.N, "%s: regs", d.name);
    CHECK(J * groups == d.K, "%s: slots", d.name);
    for (int x : v.A) CHECK(x >= -2 && x <= 2, "%s t%d: |A| > 2", d.name, t);
    for (int x : v.B) CHECK(x >= -2 && x <= 2, "%s t%d: |B| > 2", d.name, t);
    for (int x : v.D) CHECK(x > -512 && x < 512, "%s t%d: |D| >= 512", d.name, t);

    // rows pairwise distinct, columns pairwise distinct, D != D^T
    std::set<std::vector<int>> rows, cols;
    bool symmetric = true;
    for (int i = 0; i < d.M; ++i) {
        std::vector<int> row, col;
        for (int j = 0; j < d.N; ++j) {
            row.push_back(v.D[(size_t)i * d.N + j]);
            col.push_back(v.D[(size_t)j * d.N + i]);
            if (row.back() != col.back()) symmetric = false;
        }
        rows.insert(row);
        cols.insert(col);
    }
    CHECK((int)rows.size() == d.M, "%s t%d: repeated row", d.name, t);
    CHECK((int)cols.size() == d.N, "%s t%d: repeated column", d.name, t);
    CHECK(!symmetric, "%s t%d: D == D^T", d.name, t);

    // the result as the lanes' packed fragments give it
    for (int l = 0; l < cusweep::kLanes; ++l)
        for (int r = 0; r < d.regs; ++r) {
            const int row = cusweep::result_row(p, l, r), col = l % d.N;
            CHECK(row >= 0 && row < d.M, "%s: row map", d.name);
            int sum = 0;
            for (int h = 0; h < groups; ++h)
                for (int j = 0; j < J; ++j)
                    sum += decode(d.elem, &v.a_frag[(size_t)(row + d.M * h) * fb + (size_t)j * eb]) *
                           decode(d.elem, &v.b_frag[(size_t)(col + d.M * h) * fb + (size_t)j * eb]);
            uint32_t bits;
            if (d.int_result) {
                bits = (uint32_t)sum;
            } else {
                const float f = (float)sum;
                std::memcpy(&bits, &f, 4);
            }
            CHECK(bits == v.expected[(size_t)l * d.regs + r],
                  "%s t%d lane %d reg %d: expected fragment", d.name, t, l, r);
        }

    // the blob holds exactly these fragments at the offsets the kernel uses
    const uint8_t *at = blob.data() + cusweep::test_offset(p, t);
    CHECK(cusweep::test_offset(p, t) + cusweep::test_bytes(p) <= (int)blob.size(),
          "%s t%d: past the blob", d.name, t);
    CHECK(std::memcmp(at, v.a_frag.data(), v.a_frag.size()) == 0, "%s: blob A", d.name);
    at += v.a_frag.size();
    CHECK(std::memcmp(at, v.b_frag.data(), v.b_frag.size()) == 0, "%s: blob B", d.name);
    at += v.b_frag.size();
    CHECK(std::memcmp(at, v.expected.data(), v.expected.size() * 4) == 0,
          "%s: blob expected", d.name);
}

}  // namespace

int main() {
    const std::vector<uint8_t> blob = cusweep::build_table();
    CHECK((int)blob.size() == cusweep::kTableBytes, "blob size");
    for (int p = 0; p < cusweep::kPipes; ++p)
        for (int t = 0; t < cusweep::kTests; ++t) check_test(p, t, blob);
    if (failures) {
        std::fprintf(stderr, "sweep_table_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("sweep_table_check: %d pipes x %d tests ok, %d table bytes\n",
                cusweep::kPipes, cusweep::kTests, cusweep::kTableBytes);
    return 0;
}
