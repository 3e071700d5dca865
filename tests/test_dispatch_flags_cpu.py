"""CPU: csrc/dispatch_flags.h, the launchers' one way from run-time flags to template parameters, built with the host compiler.

For N = 1 ... 4 and every one of the 2^N bit patterns, dispatch_flags<N>(bits, f) must call f exactly once, with N tags, tag k
carrying bit k of the pattern as a compile-time constant (read here through a template parameter, as a launcher reads it), in bit
order; flag_bits(b0, b1, ...) must put its k-th argument at bit k."""
import ctypes
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "luciddreamer_amd", "csrc")

WRAPPER = r"""
#include "dispatch_flags.h"
template <bool... B> struct Pattern {               // the tags as template arguments: compile-time constants or no build
    static unsigned bits() { unsigned v = 0, k = 0; ((v |= (B ? 1u : 0u) << k++), ...); return v; }
};
// out[0] = calls, out[1] = tags of the last call, out[2] = their values, tag k at bit k
template <int N> static void run(unsigned bits, int* out)
{
    out[0] = out[1] = out[2] = 0;
    lr::dispatch_flags<N>(bits, [&](auto... tag) {
        static_assert((std::is_same<decltype(tag), std::bool_constant<decltype(tag)::value>>::value && ...), "std::bool_constant tags");
        out[0]++;
        out[1] = (int)sizeof...(tag);
        out[2] = (int)Pattern<tag.value...>::bits();
    });
}
extern "C" int df_run(int n, unsigned bits, int* out)
{
    switch (n) {
        case 1: run<1>(bits, out); return 0;
        case 2: run<2>(bits, out); return 0;
        case 3: run<3>(bits, out); return 0;
        case 4: run<4>(bits, out); return 0;
    }
    return -1;
}
extern "C" unsigned df_bits(int b0, int b1, int b2, int b3) { return lr::flag_bits(b0 != 0, b1 != 0, b2 != 0, b3 != 0); }
static_assert(lr::flag_bits(false, true) == 2u && lr::flag_bits(true, false, true) == 5u, "bit k = argument k");
"""


@pytest.fixture(scope="module")
def df(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / c++ / clang++) on this machine")
    d = tmp_path_factory.mktemp("dispatch_flags")
    src, so = d / "df.cpp", d / "libdf.so"
    src.write_text(WRAPPER)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)])
    return ctypes.CDLL(str(so))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_every_pattern_reaches_the_callback_once_in_bit_order(df, n):
    out = (ctypes.c_int * 3)()
    for bits in range(1 << n):
        assert df.df_run(n, bits, out) == 0
        assert list(out) == [1, n, bits], (n, bits, list(out))
    # bits beyond the N-th are not read
    assert df.df_run(n, (1 << n) | 1, out) == 0 and list(out) == [1, n, 1]


def test_flag_bits_puts_argument_k_at_bit_k(df):
    df.df_bits.restype = ctypes.c_uint
    for bits in range(16):
        assert df.df_bits(*[(bits >> k) & 1 for k in range(4)]) == bits
