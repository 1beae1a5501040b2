// Fill pattern of the HBM copy check: the one definition that
// fill_pattern_kernel writes and that verify_pattern_kernel (probe_kernels.h)
// and tests/native/hbm_pattern_check.cpp compare against.  Plain C++17, no
// HIP: constexpr functions, usable from device and host code alike.
//
// Element i of a float4 buffer is
//     x = i & 0xFFFF, y = (i >> 16) & 0xFFFF, z = (i >> 32) & 0xFFFF,
//     w = x + 0.5
// Every component is below 2^16 + 1 with at most one fractional bit, so it is
// exact in fp32, and (x, y, z) spell the low 48 bits of i: the pattern is
// injective for i < 2^48.  A copy displaced by ANY distance below 2^48
// elements, a power of two included (a stuck address bit), differs from the
// pattern in at least one component.  (A pattern of period 2^16 elements
// cannot see a displacement by a multiple of 1 MiB, and the one-shot copy's
// grid stride is such a multiple at every size the probe ships with.)
//
// Comparisons are on the bit patterns, not with ==: -0.0f == 0.0f, and
// element 0 holds three zeros.
#pragma once

#include <cstdint>

namespace hbmpattern {

// Byte that the checks fill a destination with before the copy.  Four of
// them are the float -2.87e-16 (0xA5A5A5A5): negative, so no pattern value.
constexpr int kPoisonByte = 0xA5;

// Elements for which the pattern is injective.
constexpr uint64_t kPeriod = (uint64_t)1 << 48;

struct Value {
    float x, y, z, w;
};

constexpr Value value(uint64_t i) {
    const float x = (float)(i & 0xFFFF);
    return {x, (float)((i >> 16) & 0xFFFF), (float)((i >> 32) & 0xFFFF),
            x + 0.5f};
}

constexpr uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// True when (x, y, z, w) is bit for bit the pattern's element i.
constexpr bool matches(uint64_t i, float x, float y, float z, float w) {
    const Value v = value(i);
    return bits(x) == bits(v.x) && bits(y) == bits(v.y) &&
           bits(z) == bits(v.z) && bits(w) == bits(v.w);
}

static_assert(matches(0x123456789ABCull, (float)0x9ABC, (float)0x5678,
                      (float)0x1234, (float)0x9ABC + 0.5f),
              "fields of the pattern");
static_assert(!matches(0, -0.0f, 0.0f, 0.0f, 0.5f), "compares bits, not values");

}  // namespace hbmpattern
