// Stand-alone check of native/valu_table.h under the sanitizers: generates
// every set's table, checks the layout's bounds and re-derives every expected
// word from the packed operands; for the lane-local ops with a second,
// integer-only statement of the op where one is short.
#include <cstdio>
#include <cstdlib>

#include "valu_table.h"

using namespace valusweep;

static int failures = 0;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

int main() {
    size_t words_checked = 0;
    for (int set = 0; set < kSets; ++set) {
        const std::vector<uint8_t> table = build_table(set);
        CHECK((int)table.size() == table_bytes(set));
        CHECK(table_bytes(set) % 16 == 0 && table_bytes(set) <= lds_bytes(set));
        const int L = lanes(set);
        for (int op = 0; op < n_ops(set); ++op) {
            const OpDesc &d = desc(set, op);
            const int NI = in_words(set, op), R = regs(set, op);
            CHECK(R >= 1 && R <= 4 && NI >= 1 && NI <= 8);
            for (int t = 0; t < n_tests(set); ++t) {
                const int off = test_offset(set, op, t);
                CHECK(off >= 0 && off + test_bytes(set, op) <= table_bytes(set));
                std::vector<uint32_t> in((size_t)L * NI), want((size_t)L * R),
                    again((size_t)L * R, 0);
                std::memcpy(in.data(), table.data() + off, in.size() * 4);
                std::memcpy(want.data(), table.data() + off + in.size() * 4, want.size() * 4);
                if (set == kTrans) {
                    // recorded: the words are the file's, in its order
                    const TestVector v = make_test(set, op, t);
                    CHECK(v.expected == want);
                } else {
                    expected_of(set, op, in.data(), again.data());
                    CHECK(again == want);
                }
                // integer-only restatements
                for (int l = 0; l < L && set != kTrans; ++l) {
                    const uint32_t *i = &in[(size_t)l * NI], *o = &want[(size_t)l * R];
                    if (d.kind == MUL_HI_U32 || d.kind == S_MUL_HI_U32) {
                        // schoolbook 16-bit limbs
                        const uint64_t a0 = i[0] & 0xFFFF, a1 = i[0] >> 16, b0 = i[1] & 0xFFFF,
                                       b1 = i[1] >> 16;
                        const uint64_t mid = a1 * b0 + (a0 * b0 >> 16), mid2 = a0 * b1 + (mid & 0xFFFF);
                        CHECK(o[0] == (uint32_t)(a1 * b1 + (mid >> 16) + (mid2 >> 16)));
                    }
                    if (d.kind == BITOP3_96 || d.kind == BITOP3_E8) {
                        const uint32_t tt = d.kind == BITOP3_96 ? 0x96 : 0xE8;
                        uint32_t r = 0;
                        for (int bit = 0; bit < 32; ++bit) {
                            const uint32_t idx = (i[0] >> bit & 1) << 2 | (i[1] >> bit & 1) << 1 |
                                                 (i[2] >> bit & 1);
                            r |= (tt >> idx & 1) << bit;
                        }
                        CHECK(o[0] == r);
                    }
                    if (d.kind == S_ADD_ADDC_U32) {
                        const uint32_t lo = i[0] + i[2], carry = lo < i[0];
                        CHECK(o[0] == lo && o[1] == i[1] + i[3] + carry);
                    }
                }
                words_checked += want.size();
            }
        }
    }
    if (failures) return 1;
    std::printf("ok: %zu expected words\n", words_checked);
    return 0;
}
