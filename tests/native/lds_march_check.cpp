// Stand-alone check of native/lds_march.h, built and run by
// tests/test_lds_sweep.py with -fsanitize=address,undefined.  Runs the
// header's schedule, thread by thread as lds_sweep_kernel does, on a host
// model of one CU's LDS with injectable faults, and checks what the
// schedule covers, which wave touches what, the transposed read's known
// answer and what each path and pattern finds.  Exit 0 = all good.
//
// A step is modelled as a GPU runs it: every read of the step before any of
// its writes (tests/native/hbm_march_check.cpp: "concurrent").
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hbm_march.h"
#include "lds_march.h"

namespace {

using hbmmarch::Element;
namespace lm = ldsmarch;

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
    enum Kind { kNone, kStuck0, kStuck1, kAlias } kind = kNone;
    uint32_t element = 0;  // kAlias: this element lands in element + distance
    int word = 0, bit = 0;
    long distance = 0;
};

// lds_bytes of LDS; every access is bounds-checked (at() throws).
class Lds {
  public:
    Lds(uint32_t bytes, Fault fault) : bytes_(bytes, 0xEE), fault_(fault) {}
    void read(uint32_t off, uint32_t len, void *out) const {
        for (uint32_t i = 0; i < len; ++i) {
            const uint32_t a = off + i;
            uint8_t b = bytes_.at(map(a));
            if (a / 16 == fault_.element && (int)(a % 16 / 4) == fault_.word &&
                (int)(a % 4) == fault_.bit / 8) {
                if (fault_.kind == Fault::kStuck0) b &= (uint8_t)~(1u << fault_.bit % 8);
                if (fault_.kind == Fault::kStuck1) b |= (uint8_t)(1u << fault_.bit % 8);
            }
            static_cast<uint8_t *>(out)[i] = b;
        }
    }
    void write(uint32_t off, uint32_t len, const void *in) {
        for (uint32_t i = 0; i < len; ++i)
            bytes_.at(map(off + i)) = static_cast<const uint8_t *>(in)[i];
    }
    void flip(uint32_t element, uint32_t word, uint32_t bit) {
        bytes_.at(element * 16 + word * 4 + bit / 8) ^= (uint8_t)(1u << bit % 8);
    }
    uint32_t size() const { return (uint32_t)bytes_.size(); }

  private:
    uint32_t map(uint32_t a) const {
        if (fault_.kind == Fault::kAlias && a / 16 == fault_.element)
            return (uint32_t)((long)a + fault_.distance * 16);
        return a;
    }
    std::vector<uint8_t> bytes_;
    Fault fault_;
};

// One flipped bit after a step, as the kernel's corruption hook.
struct Hook {
    int step = -1;
    uint32_t element = 0, word = 0, bit = 0;
};

struct Result {
    long mismatches = 0;
    uint32_t first_element = ~0u, first_word = 0;
    bool covered_once = true;    // every step: each covered byte exactly once
    bool other_wave = true;      // reader of step s + 1 is not the writer of s
    bool threads_agree = true;   // thread_of_item names the thread that ran it
};

struct Tracker {
    std::vector<int> touched, writer, new_writer;
    explicit Tracker(uint32_t bytes)
        : touched(bytes, 0), writer(bytes, -1), new_writer(bytes, -1) {}
    void begin_step() {
        std::fill(touched.begin(), touched.end(), 0);
        new_writer = writer;
    }
    void end_step(uint32_t covered, Result &r) {
        for (uint32_t b = 0; b < covered; ++b)
            if (touched[b] != 1) r.covered_once = false;
        writer = new_writer;
    }
};

void note(Result &r, uint32_t element, uint32_t word) {
    ++r.mismatches;
    if (element < r.first_element) {
        r.first_element = element;
        r.first_word = word;
    }
}

// What ds_read_b64_tr_b16 does, written from the instruction's description
// and not from the header: within each group of 16 consecutive lanes, lane
// 4q + p supplies the address of row q, columns 4p .. 4p + 3 (8 bytes);
// lane i receives column i of rows 0..3, row q in its element q.
void hardware_tr16(const Lds &lds, const uint32_t address[64], uint16_t out[64][4]) {
    for (int g = 0; g < 4; ++g)
        for (int i = 0; i < 16; ++i)
            for (int q = 0; q < 4; ++q) {
                const uint32_t row = address[16 * g + 4 * q + i / 4];
                lds.read(row + 2 * (i % 4), 2, &out[16 * g + i][q]);
            }
}

// One round of one path with one pattern, thread by thread.
Result run_path(Lds &lds, int path, int pattern, uint64_t block, uint64_t seed,
                Hook hook = Hook{}) {
    Result res;
    const uint32_t lds_bytes = lds.size(), elems = lds_bytes / 16;
    const uint32_t W = lm::access_bytes(path);
    Tracker track(lds_bytes);
    auto pat = [&](uint32_t e) {
        return hbmmarch::pattern(pattern, seed, lm::pattern_index(path, block, elems, e));
    };
    for (int step = 0; step < lm::path_steps(path); ++step) {
        track.begin_step();
        // step 0 of dma and tr16 fills everything; their later steps and
        // the march work on the covered prefix at the path's width
        const bool fill = !lm::is_march(path) && step == 0;
        const uint32_t width = fill ? 16 : W;
        const uint32_t covered = fill ? lds_bytes : lm::covered_bytes(path, lds_bytes);
        const uint32_t n = covered / width;
        const int rot_step = fill ? 0 : step;

        if (path == lm::kDma && step == 1) {
            // the fill: wave w, instruction k, lane l
            for (uint32_t w = 0; w < (uint32_t)lm::kWaves; ++w)
                for (uint32_t k = 0; k < lm::dma_instructions(lds_bytes, w); ++k)
                    for (uint32_t l = 0; l < (uint32_t)lm::kWaveSize; ++l) {
                        const uint32_t e = 64 * lm::dma_kib(w, k) + l;
                        const Element v = hbmmarch::pattern(pattern, seed, e);
                        lds.write(16 * e, 16, &v);
                        for (uint32_t b = 16 * e; b < 16 * e + 16; ++b) {
                            ++track.touched.at(b);
                            track.new_writer[b] = (int)w;
                        }
                    }
        } else if (path == lm::kTr16 && step == 1) {
            for (uint32_t k = 0; k < lm::tr16_rounds(lds_bytes); ++k)
                for (uint32_t w = 0; w < (uint32_t)lm::kWaves; ++w) {
                    uint32_t address[64];
                    uint16_t got[64][4];
                    for (uint32_t l = 0; l < 64; ++l)
                        address[l] = lm::tr16_address(64 * w + l, k);
                    hardware_tr16(lds, address, got);
                    for (uint32_t l = 0; l < 64; ++l) {
                        const uint32_t t = 64 * w + l;
                        for (uint32_t b = 0; b < 8; ++b) ++track.touched.at(address[l] + b);
                        bool bad = false;
                        for (uint32_t q = 0; q < 4; ++q) {
                            const uint32_t off = lm::kTr16Bytes * k + lm::tr16_source(t, q);
                            const uint32_t want = lm::half_of(pat(off / 16), off % 16);
                            if (got[l][q] != want && !bad) {
                                bad = true;  // one access, one mismatch
                                note(res, off / 16, off % 16 / 4);
                            }
                        }
                    }
                }
        } else {
            for (int phase = 0; phase < 2; ++phase)  // all reads, then all writes
                for (uint32_t t = 0; t < (uint32_t)lm::kThreads; ++t)
                    for (uint32_t a = lm::lane_residue(rot_step, t); a < n; a += lm::kThreads) {
                        const uint32_t j = lm::step_access(path, step, n, a);  // its own inverse
                        if (lm::thread_of_access(rot_step, a) != t ||
                            (!fill && lm::thread_of_item(path, step, n, j) != t))
                            res.threads_agree = false;
                        const uint32_t off = a * width, e = off / 16, w0 = off % 16 / 4;
                        const Element v = lm::expected_of(path, pat(e), step);
                        const Element x = lm::to_write_of(path, pat(e), step);
                        if (phase == 0) {
                            for (uint32_t b = off; b < off + width; ++b) {
                                ++track.touched.at(b);
                                if (!fill && lm::step_reads(path, step) &&
                                    track.writer[b] == (int)(t / 64))
                                    res.other_wave = false;
                            }
                            if (!fill && lm::step_reads(path, step)) {
                                uint32_t got[4] = {0, 0, 0, 0};
                                lds.read(off, width, got);
                                for (uint32_t w = 0; w < width / 4; ++w)
                                    if (got[w] != v.w[w0 + w]) {
                                        note(res, e, w0 + w);
                                        break;
                                    }
                            }
                        } else if (fill || lm::step_writes(path, step)) {
                            lds.write(off, width, &x.w[w0]);
                            for (uint32_t b = off; b < off + width; ++b)
                                track.new_writer[b] = (int)(t / 64);
                        }
                    }
        }
        track.end_step(covered, res);
        if (hook.step == step) lds.flip(hook.element, hook.word, hook.bit);
    }
    return res;
}

int fixed_or(int path, int pattern) {
    return path == lm::kDma ? (int)hbmmarch::kRandom
           : path == lm::kTr16 ? (int)hbmmarch::kAddress : pattern;
}

const char *pname(int p) { return lm::kPathNames[p]; }

}  // namespace

int main() {
    const uint64_t seed = 0x5EED;
    const uint32_t sizes[] = {16, 2048, 2064, 65536, 67584, 163840};

    // the known answer of the transposed read, against an independently
    // written transposition: a 2048-byte round is 16 tiles of 4 rows x 16
    // columns of 16-bit values, tile g to lanes 16g..16g+15 column-wise
    for (uint32_t t = 0; t < 256; ++t)
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t tile = t / 16, column = t % 16, row = q;
            CHECK(lm::tr16_source(t, q) == tile * 128 + (row * 16 + column) * 2,
                  "tr16_source(%u, %u)", t, q);
        }
    for (uint32_t t = 0; t < 256; ++t)
        CHECK(lm::tr16_address(t, 3) == 3 * 2048 + 8 * t, "tr16_address(%u)", t);

    for (uint32_t lds_bytes : sizes) {
        const uint32_t elems = lds_bytes / 16;
        // the whole matrix of faults at the small sizes, where every branch
        // of the schedule is taken already; one of each kind at the large
        const bool small = lds_bytes <= 2064;
        const std::vector<uint32_t> words = small ? std::vector<uint32_t>{0, 3} : std::vector<uint32_t>{3};
        const std::vector<uint32_t> bits = small ? std::vector<uint32_t>{0, 15, 16, 31} : std::vector<uint32_t>{16};

        // the dma tiling: every whole KiB once, nothing else
        std::vector<int> kib_count(lds_bytes / 1024 + 1, 0);
        for (uint32_t w = 0; w < 4; ++w)
            for (uint32_t k = 0; k < lm::dma_instructions(lds_bytes, w); ++k)
                ++kib_count.at(lm::dma_kib(w, k));
        for (uint32_t i = 0; i < lds_bytes / 1024; ++i)
            CHECK(kib_count[i] == 1, "%u bytes: KiB %u filled %d times", lds_bytes, i, kib_count[i]);
        CHECK(kib_count[lds_bytes / 1024] == 0, "%u bytes: the fill passes the last whole KiB", lds_bytes);
        CHECK(lm::covered_bytes(lm::kDma, lds_bytes) == lds_bytes / 1024 * 1024 &&
                  lm::covered_bytes(lm::kTr16, lds_bytes) == lds_bytes / 2048 * 2048 &&
                  lm::covered_bytes(lm::kB64, lds_bytes) == lds_bytes,
              "%u bytes: covered bytes", lds_bytes);

        for (int path = 0; path < lm::kPaths; ++path) {
            const uint32_t covered = lm::covered_bytes(path, lds_bytes);
            // clean LDS, every pattern the path can run, two blocks
            for (int p = 0; p < hbmmarch::kPatterns; ++p) {
                if (fixed_or(path, p) != p) continue;
                for (uint64_t block : {(uint64_t)0, (uint64_t)255}) {
                    Lds lds(lds_bytes, Fault{});
                    const Result r = run_path(lds, path, p, block, seed);
                    CHECK(r.mismatches == 0, "%u bytes %s %s: clean LDS fails (%ld)", lds_bytes,
                          pname(path), hbmmarch::kPatternNames[p], r.mismatches);
                    CHECK(r.covered_once, "%u bytes %s: a step misses or repeats a byte", lds_bytes, pname(path));
                    CHECK(r.threads_agree, "%u bytes %s: thread_of_item disagrees", lds_bytes, pname(path));
                    if (path != lm::kTr16)  // the transposed read is not rotated
                        CHECK(r.other_wave, "%u bytes %s: a wave reads back its own write", lds_bytes, pname(path));
                }
            }
            if (!covered) continue;
            const uint32_t n_el = covered / 16;

            // a flipped bit after each step that a reading step follows
            for (int step = 0; step < lm::path_steps(path); ++step) {
                if (!lm::step_is_followed_by_read(path, step)) continue;
                for (uint32_t element : {0u, n_el / 2, n_el - 1})
                    for (uint32_t word : words)
                        for (uint32_t bit : bits) {
                            Lds lds(lds_bytes, Fault{});
                            Hook h;
                            h.step = step;
                            h.element = element;
                            h.word = word;
                            h.bit = bit;
                            const Result r = run_path(lds, path, fixed_or(path, hbmmarch::kChecker), 3, seed, h);
                            CHECK(r.mismatches == 1 && r.first_element == element && r.first_word == word,
                                  "%u bytes %s: flip after step %d at %u.%u bit %u: %ld mismatches, first %u.%u",
                                  lds_bytes, pname(path), step, element, word, bit, r.mismatches,
                                  r.first_element, r.first_word);
                        }
            }

            // a stuck bit
            for (Fault::Kind kind : {Fault::kStuck0, Fault::kStuck1})
                for (uint32_t element : {0u, n_el - 1})
                    for (int word : small ? std::vector<int>{0, 2} : std::vector<int>{2})
                        for (int bit : small ? std::vector<int>{0, 9, 31} : std::vector<int>{9}) {
                            Fault f;
                            f.kind = kind;
                            f.element = element;
                            f.word = word;
                            f.bit = bit;
                            for (int p = 0; p < hbmmarch::kPatterns; ++p) {
                                if (fixed_or(path, p) != p) continue;
                                Lds lds(lds_bytes, f);
                                const long got = run_path(lds, path, p, 1, seed).mismatches;
                                if (lm::is_march(path)) {
                                    // p and ~p are both read: every pattern sees it
                                    CHECK(got >= 1, "%u bytes %s %s: misses stuck-at-%d at %u.%d bit %d", lds_bytes,
                                          pname(path), hbmmarch::kPatternNames[p], kind == Fault::kStuck1, element, word, bit);
                                } else {
                                    // one value per cell: seen when the value differs
                                    const Element v = hbmmarch::pattern(p, seed, lm::pattern_index(path, 1, elems, element));
                                    const bool holds = v.w[word] >> bit & 1;
                                    CHECK(got == (holds != (kind == Fault::kStuck1)),
                                          "%u bytes %s: stuck-at-%d at %u.%d bit %d gives %ld", lds_bytes, pname(path),
                                          kind == Fault::kStuck1, element, word, bit, got);
                                }
                            }
                        }

            // two elements that share a cell
            for (long distance : {1L, 16L, 4096L}) {
                if ((long)n_el <= distance) continue;
                Fault f;
                f.kind = Fault::kAlias;
                f.element = 0;
                f.distance = distance;
                for (int p : {(int)hbmmarch::kAddress, (int)hbmmarch::kRandom}) {
                    if (fixed_or(path, p) != p) continue;
                    Lds lds(lds_bytes, f);
                    CHECK(run_path(lds, path, p, 2, seed).mismatches >= 1,
                          "%u bytes %s %s: misses an alias at distance %ld", lds_bytes, pname(path),
                          hbmmarch::kPatternNames[p], distance);
                }
            }
        }
    }

    // corruptible steps: the march 0..2, dma only after its fill, tr16 after its write
    CHECK(lm::step_is_followed_by_read(lm::kB128, 0) && lm::step_is_followed_by_read(lm::kB32, 2) &&
              !lm::step_is_followed_by_read(lm::kB64, 3) && !lm::step_is_followed_by_read(lm::kDma, 0) &&
              lm::step_is_followed_by_read(lm::kDma, 1) && !lm::step_is_followed_by_read(lm::kDma, 2) &&
              lm::step_is_followed_by_read(lm::kTr16, 0) && !lm::step_is_followed_by_read(lm::kTr16, 1),
          "which steps a reading step follows");

    if (failures) {
        std::fprintf(stderr, "lds_march_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("lds_march_check: ok\n");
    return 0;
}
