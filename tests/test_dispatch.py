"""plan_amd/csrc/dispatch.h on the host: a run-time value reaches the compile-time constant of its own name.

The launch sites of ops_join / ops_merge / ops_agg / scan_kernels choose a kernel's template instance through dispatch_int /
dispatch_bool; a value that reached another constant would launch another instance. The header has no HIP in it, so a plain
g++ program checks it: every listed value reaches its own constant, an unlisted one the LAST of the list (a ladder's final
else), both booleans map, and a nested pair hands back what the inner lambda returns.
"""
import pathlib
import shutil
import subprocess

import pytest

CSRC = pathlib.Path(__file__).resolve().parents[1] / "plan_amd" / "csrc"

PROGRAM = r"""
#include "dispatch.h"
#include <cstdio>
#include <initializer_list>

static int fails = 0;
#define EXPECT(got, want) \
    do { const long g_ = (got), w_ = (want); if (g_ != w_) { std::printf("line %d: %s = %ld, expected %ld\n", __LINE__, #got, g_, w_); fails++; } } while (0)

template <int... Vs>
static int reached(int v) { return ph::dispatch_int<Vs...>(v, [](auto C) { static_assert(std::is_same_v<typename decltype(C)::value_type, int>); return C(); }); }

template <int A, int B> struct Inst { static constexpr int id = A * 100 + B; };

int main() {
    for (int v : {4, 8}) EXPECT((reached<4, 8>(v)), v);
    for (int v : {4, 1, 8}) EXPECT((reached<4, 1, 8>(v)), v);
    for (int v : {0, 1, 2, 3}) EXPECT((reached<0, 1, 2, 3>(v)), v);
    // not listed: the last of the list
    for (int v : {-1, 0, 1, 2, 5, 16, 1 << 30}) EXPECT((reached<4, 8>(v)), 8);
    for (int v : {-1, 0, 2, 9}) EXPECT((reached<4, 1, 8>(v)), 8);
    for (int v : {-1, 4, 7}) EXPECT((reached<0, 1, 2, 3>(v)), 3);
    for (int v : {0, 3, 8}) EXPECT((reached<2, 1>(v)), 1);
    EXPECT((reached<7>(7)), 7);
    EXPECT((reached<7>(0)), 7);

    EXPECT(ph::dispatch_bool(true, [](auto B) { return B() ? 10 : 20; }), 10);
    EXPECT(ph::dispatch_bool(false, [](auto B) { return B() ? 10 : 20; }), 20);

    // a nested pair: the constants are usable as template arguments and the inner lambda's value comes back
    for (int kw : {4, 8, 5})
        for (int sel = 0; sel < 2; sel++) {
            const int got = ph::dispatch_int<4, 8>(kw, [&](auto KW) { return ph::dispatch_bool(sel != 0, [&](auto SEL) { return Inst<KW(), SEL()>::id; }); });
            EXPECT(got, (kw == 4 ? 4 : 8) * 100 + sel);
        }
    for (int a : {4, 8}) for (int b : {4, 8}) {
        const long got = ph::dispatch_int<4, 8>(a, [&](auto A) { return ph::dispatch_int<4, 8>(b, [&](auto B) { return (long)Inst<A(), B()>::id; }); });
        EXPECT(got, a * 100 + b);
    }
    // a void body is called exactly once
    int calls = 0;
    ph::dispatch_int<1, 2, 3>(2, [&](auto C) { calls += C(); });
    EXPECT(calls, 2);
    ph::dispatch_bool(true, [&](auto) { calls++; });
    EXPECT(calls, 3);
    if (!fails) std::printf("dispatch ok\n");
    return fails ? 1 : 0;
}
"""


def test_dispatch_reaches_its_own_constant(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the host-only check of dispatch.h needs a C++17 host compiler")
    src = tmp_path / "dispatch_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "dispatch_check"
    cc = subprocess.run([gxx, "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "dispatch ok"
