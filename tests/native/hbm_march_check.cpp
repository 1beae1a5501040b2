// Stand-alone check of native/hbm_march.h, built and run by
// tests/test_hbm_scrub.py with -fsanitize=address,undefined.  Runs the
// header's march on a host array behind a small faulty-memory model and
// checks what each pattern finds and what it misses.  Exit 0 = all good.
//
// Two orders of one step are modelled:
//   sequential  element after element, each read and then written: the
//               textbook march, one work item at a time;
//   concurrent  every read of the step before any of its writes: the other
//               extreme, and what a GPU does to neighbours in flight (the
//               kernel itself loads a thread's four elements before it
//               stores any of them).
// A stuck or slow bit is found in either order by every pattern.  Two
// addresses that share one cell are found by every pattern in sequential
// order, the march's classical argument; in concurrent order only a pattern
// whose value depends on the address finds them.  A real launch lies
// between the two: an aliased pair is handled either at different times
// (found by every pattern) or in the same window of loads in flight (then
// `solid` and `checker` miss it).  So `solid` and `checker` alone MAY miss
// an alias on a GPU; that is what `address` and `random` are for.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hbm_march.h"
#include "hbm_pattern.h"

namespace {

using hbmmarch::Element;

int failures = 0;

#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);          \
            ++failures;                        \
        }                                      \
    } while (0)

struct Fault {
    enum Kind { kNone, kStuck0, kStuck1, kNoRise, kAlias } kind = kNone;
    uint64_t cell = 0;  // kAlias: the address that lands in cell ^ (1 << k)
    int word = 0, bit = 0, k = 0;
};

class Memory {
  public:
    Memory(size_t n, Fault fault) : cells_(n), fault_(fault) {
        std::memset(cells_.data(), hbmpattern::kPoisonByte, n * sizeof(Element));
    }
    Element read(uint64_t addr) const {
        Element e = cells_.at(map(addr));
        if (map(addr) == fault_.cell) {
            if (fault_.kind == Fault::kStuck0) e.w[fault_.word] &= ~mask();
            if (fault_.kind == Fault::kStuck1) e.w[fault_.word] |= mask();
        }
        return e;
    }
    void write(uint64_t addr, Element e) {
        Element &cell = cells_.at(map(addr));
        if (fault_.kind == Fault::kNoRise && map(addr) == fault_.cell &&
            !(cell.w[fault_.word] & mask()))
            e.w[fault_.word] &= ~mask();  // the bit cannot go from 0 to 1
        cell = e;
    }

  private:
    uint32_t mask() const { return 1u << fault_.bit; }
    uint64_t map(uint64_t addr) const {
        if (fault_.kind == Fault::kAlias && addr == fault_.cell)
            return addr ^ ((uint64_t)1 << fault_.k);
        return addr;
    }
    std::vector<Element> cells_;
    Fault fault_;
};

// The march of hbm_march.h with the given patterns; returns the mismatches.
long run_march(Memory &mem, uint64_t n, const std::vector<int> &patterns,
               uint64_t seed, bool concurrent) {
    long bad = 0;
    for (int p : patterns)
        for (int step = 0; step < hbmmarch::kSteps; ++step) {
            auto read = [&](uint64_t i) {
                if (hbmmarch::step_reads(step) &&
                    !hbmmarch::equal(mem.read(i),
                                     hbmmarch::expected(p, seed, step, i)))
                    ++bad;
            };
            auto write = [&](uint64_t i) {
                if (hbmmarch::step_writes(step))
                    mem.write(i, hbmmarch::to_write(p, seed, step, i));
            };
            if (concurrent) {
                for (uint64_t j = 0; j < n; ++j)
                    read(hbmmarch::step_element(step, n, j));
                for (uint64_t j = 0; j < n; ++j)
                    write(hbmmarch::step_element(step, n, j));
            } else {
                for (uint64_t j = 0; j < n; ++j) {
                    const uint64_t i = hbmmarch::step_element(step, n, j);
                    read(i);
                    write(i);
                }
            }
        }
    return bad;
}

long march(uint64_t n, Fault fault, const std::vector<int> &patterns,
           bool concurrent, uint64_t seed = 0x5EED) {
    Memory mem(n, fault);
    return run_march(mem, n, patterns, seed, concurrent);
}

const char *name(int p) { return hbmmarch::kPatternNames[p]; }

}  // namespace

int main() {
    static_assert(sizeof(Element) == 16, "one 16-byte element");
    const uint64_t n = 4099;  // a few thousand, and no power of two
    const std::vector<int> all = {hbmmarch::kAddress, hbmmarch::kSolid,
                                  hbmmarch::kChecker, hbmmarch::kRandom};

    // the table of the header's comment
    for (int step = 0; step < hbmmarch::kSteps; ++step) {
        CHECK(hbmmarch::step_reads(step) == (step != 0), "step %d reads", step);
        CHECK(hbmmarch::step_writes(step) == (step != 3), "step %d writes", step);
        CHECK(hbmmarch::step_descends(step) == (step == 2), "step %d order", step);
    }
    CHECK(hbmmarch::step_element(2, n, 0) == n - 1 &&
              hbmmarch::step_element(2, n, n - 1) == 0 &&
              hbmmarch::step_element(1, n, 5) == 5,
          "work item j of a descending step handles n - 1 - j");
    for (int p : all)
        for (uint64_t i : {(uint64_t)0, (uint64_t)77, (uint64_t)0xFFFFFFFFull,
                           (uint64_t)0x100000000ull, (uint64_t)0x123456789ABull}) {
            const Element e = hbmmarch::pattern(p, 9, i);
            CHECK(hbmmarch::equal(hbmmarch::to_write(p, 9, 0, i), e), "%s: step 0 writes p", name(p));
            CHECK(hbmmarch::equal(hbmmarch::expected(p, 9, 1, i), e), "%s: step 1 expects p", name(p));
            CHECK(hbmmarch::equal(hbmmarch::expected(p, 9, 2, i), hbmmarch::inverse(e)), "%s: step 2 expects ~p", name(p));
            CHECK(hbmmarch::equal(hbmmarch::expected(p, 9, 3, i), e), "%s: step 3 expects p", name(p));
            for (int step : {1, 2})
                CHECK(hbmmarch::equal(hbmmarch::to_write(p, 9, step, i),
                                      hbmmarch::inverse(hbmmarch::expected(p, 9, step, i))),
                      "%s: step %d writes the complement of what it expects", name(p), step);
            const Element inv = hbmmarch::inverse(e);
            for (int w = 0; w < 4; ++w)
                CHECK((inv.w[w] ^ e.w[w]) == 0xFFFFFFFFu, "%s: inverse flips all 128 bits", name(p));
        }

    // address is injective across the field boundary
    const uint64_t edge[] = {0, 1, 0xFFFFFFFEull, 0xFFFFFFFFull, 0x100000000ull,
                             0x100000001ull, 0x1FFFFFFFFull, 0x200000000ull};
    for (uint64_t a : edge)
        for (uint64_t b : edge)
            CHECK((a == b) == hbmmarch::equal(hbmmarch::pattern(hbmmarch::kAddress, 0, a),
                                              hbmmarch::pattern(hbmmarch::kAddress, 0, b)),
                  "address(%llu) against address(%llu)", (unsigned long long)a,
                  (unsigned long long)b);
    for (uint64_t i : edge) {
        const Element e = hbmmarch::pattern(hbmmarch::kAddress, 0, i);
        CHECK(((uint64_t)e.w[1] << 32 | e.w[0]) == i && e.w[2] == ~e.w[0],
              "address(%llu) does not spell i", (unsigned long long)i);
    }
    // random depends on the seed and on i
    CHECK(!hbmmarch::equal(hbmmarch::pattern(hbmmarch::kRandom, 1, 5),
                           hbmmarch::pattern(hbmmarch::kRandom, 2, 5)) &&
              !hbmmarch::equal(hbmmarch::pattern(hbmmarch::kRandom, 1, 5),
                               hbmmarch::pattern(hbmmarch::kRandom, 1, 6)),
          "random ignores its seed or its index");

    for (bool concurrent : {false, true}) {
        const char *order = concurrent ? "concurrent" : "sequential";
        // fault-free memory: nothing, whichever patterns run
        CHECK(march(n, Fault{}, all, concurrent) == 0, "%s: clean memory fails", order);
        for (int p : all)
            CHECK(march(n, Fault{}, {p}, concurrent) == 0, "%s: clean memory fails %s", order, name(p));

        // a stuck or slow bit: every pattern alone sees it
        for (Fault::Kind kind : {Fault::kStuck0, Fault::kStuck1, Fault::kNoRise})
            for (uint64_t cell : {(uint64_t)0, (uint64_t)1234, n - 1})
                for (int word = 0; word < 4; ++word)
                    for (int bit : {0, 1, 10, 30, 31}) {
                        Fault f;
                        f.kind = kind;
                        f.cell = cell;
                        f.word = word;
                        f.bit = bit;
                        for (int p : all)
                            CHECK(march(n, f, {p}, concurrent) >= 1,
                                  "%s: %s misses fault kind %d at cell %llu word %d bit %d",
                                  order, name(p), (int)kind, (unsigned long long)cell, word, bit);
                        CHECK(march(n, f, all, concurrent) >= 1, "%s: all patterns miss a fault", order);
                    }

        // an address-line alias: a and a ^ (1 << k) share one cell
        for (int k : {0, 1, 5, 11}) {
            Fault f;
            f.kind = Fault::kAlias;
            f.cell = 1000;  // 1000 ^ (1 << k) < n for every k here
            f.k = k;
            for (int p : {(int)hbmmarch::kAddress, (int)hbmmarch::kRandom})
                CHECK(march(n, f, {p}, concurrent) >= 1, "%s: %s misses the alias, k = %d", order, name(p), k);
            CHECK(march(n, f, all, concurrent) >= 1, "%s: all patterns miss the alias, k = %d", order, k);
            for (int p : {(int)hbmmarch::kSolid, (int)hbmmarch::kChecker}) {
                const long got = march(n, f, {p}, concurrent);
                if (concurrent)
                    CHECK(got == 0, "concurrent: %s alone finds the alias (%ld), k = %d: "
                          "the model or the pattern changed", name(p), got, k);
                else
                    CHECK(got >= 1, "sequential: %s misses the alias, k = %d", name(p), k);
            }
        }
    }

    if (failures) {
        std::fprintf(stderr, "hbm_march_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("hbm_march_check: %llu elements ok\n", (unsigned long long)n);
    return 0;
}
