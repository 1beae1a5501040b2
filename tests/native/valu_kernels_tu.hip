// Instantiates every VALU sweep kernel, for the mnemonic test: compiled to
// gfx950 assembly, never linked or run.
#include "valu_kernels.h"

template <int... S>
void take_sets(std::integer_sequence<int, S...>, const void **out) {
    const void *k[] = {reinterpret_cast<const void *>(&valu_sweep_kernel<S>)...};
    for (int i = 0; i < (int)sizeof...(S); ++i) out[i] = k[i];
}

void valu_kernels_tu(const void **out) {
    take_sets(std::make_integer_sequence<int, valusweep::kSets>{}, out);
}
