// dispatch_flags.h -- run-time flags to template parameters, the one way the launchers do it.
// Pure C++17, no HIP: tests/test_dispatch_flags_cpu.py builds it with the host compiler.
#pragma once
#include <type_traits>

namespace lr {

// bit k = the k-th argument
template <class... B>
constexpr unsigned flag_bits(B... b)
{
    unsigned bits = 0, k = 0;
    ((bits |= (b ? 1u : 0u) << k++), ...);
    return bits;
}

// f(tag0, ..., tagN-1), called once, with bit k of `bits` as the compile-time constant tagk.value (std::bool_constant): a
// generic lambda is instantiated for all 2^N patterns from one call site, and the order of its parameters is the order of the bits:
//   dispatch_flags<2>(flag_bits(raw, aa), [&](auto raw, auto aa) { hipLaunchKernelGGL((k<raw.value, aa.value>), ...); });
template <int N, class F, class... Tags>
void dispatch_flags(unsigned bits, F&& f, Tags... tags)
{
    if constexpr (N == 0) f(tags...);
    else if (bits & 1u) dispatch_flags<N - 1>(bits >> 1, f, tags..., std::true_type{});
    else dispatch_flags<N - 1>(bits >> 1, f, tags..., std::false_type{});
}

}  // namespace lr
