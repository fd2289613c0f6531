"""plan_amd/csrc/scan_lower.h on the host: what a scan descriptor lowers to, without a device.

The header has no HIP in it, so a plain g++ program checks it, as tests/test_dispatch.py does for dispatch.h:
 * DECIMAL {>, >=, <=} FLOAT as an integer range, against brute force over every unscaled value of the column's range. The right-hand side
   is computed here as (float)((double)d / 10^scale) op k, independently of the header's cast and bisection;
 * the (type, operator) pairs that select nothing, and the two literals at the ends of int64 that cannot be stepped past;
 * normalize on Q1's charge expression and on constants that enter at other scales, and the shapes it refuses;
 * the 24-bit bound of the lean factors, the code-domain bounds, and the roles of lowcard_chain for the descriptors of
   tests/test_gpu_scan_plan_shapes.py."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

PROGRAM = r"""
#include "scan_lower.h"
#include <cstdio>
#include <initializer_list>

using namespace ph;
static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static ColView view(int32_t type, int32_t scale, int64_t mn, int64_t mx, bool nullable = false) {
    ColView c; c.type = type; c.scale = scale; c.has_range = true; c.min = mn; c.max = mx; c.nullable = nullable; return c;
}
static ph_pred pred(int32_t col, int32_t op, int32_t type, int64_t i = 0, double f = 0, int32_t scale = 0) {
    ph_pred p{}; p.col = col; p.op = op; p.k.type = type; p.k.i = i; p.k.f = f; p.k.scale = scale; return p;
}
static bool never_of(const ColView &c, const ph_pred &p) { Range r; return lower_pred(c, p, &r) == PH_OK && r.never; }

// lo <= d <= hi  <=>  (float)((double)d / 10^scale) op k, for every d of the column's range
static void float_brute(int64_t mn, int64_t mx, int scale) {
    const ColView c = view(PH_DEC64, scale, mn, mx);
    double p10 = 1; for (int i = 0; i < scale; i++) p10 *= 10;
    for (float k : {0.05f, 0.06f, 0.07f, 24.0f, 16777217.0f, -0.05f, 16777216.0f, 16777218.0f})
        for (int32_t op : {PH_GT, PH_GE, PH_LE}) {
            Range r;
            if (lower_pred(c, pred(0, op, PH_F32, 0, k), &r) != PH_OK) { std::printf("scale %d k %g op %d: not lowered\n", scale, k, op); fails++; continue; }
            for (int64_t d = mn; d <= mx; d++) {
                const float x = (float)((double)d / p10);
                const bool want = op == PH_GT ? x > k : op == PH_GE ? x >= k : x <= k;
                const bool got = !r.never && r.lo <= d && d <= r.hi;
                if (want != got) { std::printf("scale %d k %.9g op %d d %lld: want %d got %d\n", scale, k, op, (long long)d, want, got); fails++; break; }
            }
        }
}

static std::vector<ph_rpn> prog(std::initializer_list<ph_rpn> l) { return l; }
static ph_rpn COL(int32_t c) { return ph_rpn{PH_X_COL, c, 0, 0}; }
static ph_rpn K(int64_t v, int32_t s) { return ph_rpn{PH_X_CONST, -1, v, s}; }
static const ph_rpn ADD{PH_X_ADD, -1, 0, 0}, SUB{PH_X_SUB, -1, 0, 0}, MUL{PH_X_MUL, -1, 0, 0};
static Affine aff(int64_t A, int64_t B, int32_t col) { Affine a; a.A = A; a.B = B; a.col = col; return a; }

// the table of tests/test_gpu_scan_plan_shapes.py
enum { SHIP, QTY, E, D, T, K0, K1, NQ, I2, D5, NCOLS };
static std::vector<ColView> table() {
    std::vector<ColView> v(NCOLS);
    v[SHIP] = view(PH_DATE, 0, 8036, 10561); v[QTY] = view(PH_I32, 0, 1, 50); v[E] = view(PH_DEC64, 2, 90000, 10494950);
    v[D] = view(PH_DEC64, 2, 0, 10); v[T] = view(PH_DEC64, 2, 0, 8); v[K0] = view(PH_CODE8, 0, 0, 1); v[K1] = view(PH_CODE8, 0, 0, 1);
    v[NQ] = view(PH_I32, 0, -5, 60, true); v[I2] = view(PH_I32, 0, 0, 1000); v[D5] = view(PH_DEC64, 0, 5, 5);
    return v;
}
static bool norm(const std::vector<ColView> &v, const std::vector<ph_rpn> &p, Prod *out) { return normalize(v.data(), (int32_t)v.size(), p.data(), (int32_t)p.size(), out); }

struct Roles { RolesResult rc; LowcardRoles R; };
static Roles roles(const std::vector<ColView> &v, std::initializer_list<std::vector<ph_rpn>> args, std::vector<Range> ranges) {
    std::vector<AggReq> reqs;
    for (auto &a : args) {
        AggReq r; r.kind = a.empty() ? PH_A_COUNT_STAR : PH_A_SUM; r.star = a.empty();
        if (!r.star && !norm(v, a, &r.p)) { std::printf("roles: an argument does not normalise\n"); fails++; }
        reqs.push_back(r);
    }
    Roles out;
    out.rc = match_lowcard_roles(reqs, ranges, v.data(), &out.R);
    return out;
}
static bool accs(const Roles &r, std::initializer_list<int> want) {
    if (r.rc != ROLES_OK || r.R.aggs.size() != want.size()) return false;
    size_t i = 0;
    for (int w : want) if (r.R.aggs[i++].acc != w) return false;
    return true;
}

int main() {
    // ---- DECIMAL against FLOAT
    float_brute(-300, 300, 2);
    float_brute((1ll << 24) - 40, (1ll << 24) + 40, 0);   // float32 stops being exact inside the range
    float_brute(-(1ll << 24) - 40, -(1ll << 24) + 40, 0);
    const ColView dec = view(PH_DEC64, 2, -300, 300), big = view(PH_I64, 0, 0, 100), date = view(PH_DATE, 0, 0, 100), i32 = view(PH_I32, 0, 0, 100);
    // ---- operators that select nothing
    for (int32_t op : {PH_LT, PH_EQ, PH_NE}) CHECK(never_of(dec, pred(0, op, PH_F32, 0, 0.05)));
    for (int32_t op : {PH_EQ, PH_NE, PH_LT, PH_LE, PH_GE}) CHECK(never_of(dec, pred(0, op, PH_DEC64, 5, 0, 2)));
    for (int32_t op : {PH_EQ, PH_NE, PH_LT, PH_LE, PH_GT, PH_GE}) CHECK(never_of(big, pred(0, op, PH_I64, 5)));
    CHECK(never_of(date, pred(0, PH_EQ, PH_DATE, 5)));
    CHECK(never_of(date, pred(0, PH_NE, PH_DATE, 5)));
    CHECK(never_of(i32, pred(0, PH_LIKE, PH_I32, 5)));
    { Range r; CHECK(lower_pred(i32, pred(0, PH_NE, PH_I32, 5), &r) == PH_EUNSUPPORTED); }
    { Range r; CHECK(lower_pred(view(PH_I32, 0, 0, 9, true), pred(0, PH_LT, PH_I32, 5), &r) == PH_EUNSUPPORTED); }
    { Range r; CHECK(lower_pred(dec, pred(0, PH_GT, PH_DEC64, 5, 0, 3), &r) == PH_EUNSUPPORTED); }   // a literal finer than the column
    { Range r; CHECK(lower_pred(dec, pred(7, PH_GT, PH_DEC64, 5, 0, 1), &r) == PH_OK && !r.never && r.lo == 51 && r.hi == INT64_MAX && r.col == 7); }
    { Range r; CHECK(lower_pred(date, pred(0, PH_LT, PH_DATE, 5), &r) == PH_OK && r.hi == 4 && r.lo == INT64_MIN); }
    { Range r; CHECK(lower_pred(i32, pred(0, PH_LT, PH_I32, INT32_MIN), &r) == PH_OK && !r.never && r.hi == (int64_t)INT32_MIN - 1); }
    // ---- the ends of int64
    { Range r; range_of(PH_LT, INT64_MIN, &r); CHECK(r.never); }
    { Range r; range_of(PH_GT, INT64_MAX, &r); CHECK(r.never); }
    { Range r; range_of(PH_LT, INT64_MIN + 1, &r); CHECK(!r.never && r.hi == INT64_MIN); }
    { Range r; range_of(PH_GT, INT64_MAX - 1, &r); CHECK(!r.never && r.lo == INT64_MAX); }
    CHECK(never_of(view(PH_DEC64, 0, 0, 9), pred(0, PH_GT, PH_DEC64, INT64_MAX)));
    // ---- merging conjuncts
    {
        std::vector<Range> rs;
        Range a; a.col = 3; a.lo = 5; merge_range(rs, a);
        Range b; b.col = 4; b.hi = 9; merge_range(rs, b);
        Range c; c.col = 3; c.hi = 7; merge_range(rs, c);
        CHECK(rs.size() == 2 && rs[0].col == 3 && rs[0].lo == 5 && rs[0].hi == 7 && rs[1].col == 4 && !selects_nothing(rs));
        Range d; d.col = 3; d.lo = 8; merge_range(rs, d);
        CHECK(rs.size() == 2 && selects_nothing(rs));   // 8 .. 7
        std::vector<Range> ns;
        merge_range(ns, a);
        Range n; n.col = 3; n.never = true; merge_range(ns, n);
        CHECK(ns.size() == 1 && selects_nothing(ns));
    }
    CHECK(clamp32(INT64_MIN) == INT32_MIN && clamp32(INT64_MAX) == INT32_MAX && clamp32(-7) == -7);
    // ---- normalize
    const std::vector<ColView> v = table();
    const std::vector<ph_rpn> dp = prog({COL(E), K(1, 0), COL(D), SUB, MUL});
    std::vector<ph_rpn> charge = dp;
    for (ph_rpn o : {K(1, 0), COL(T), ADD, MUL}) charge.push_back(o);
    {
        Prod p;
        CHECK(norm(v, charge, &p) && p.scale == 6 && p.f.size() == 3 && p.f[0] == aff(0, 1, E) && p.f[1] == aff(100, -1, D) && p.f[2] == aff(100, 1, T));
        CHECK(norm(v, prog({COL(D), K(5, 4), ADD}), &p) && p.scale == 4 && p.f.size() == 1 && p.f[0] == aff(5, 100, D));
        CHECK(norm(v, prog({K(7, 0), COL(QTY), SUB}), &p) && p.scale == 0 && p.f[0] == aff(7, -1, QTY));
        CHECK(norm(v, prog({K(3, 1), COL(E), MUL}), &p) && p.scale == 3 && p.f.size() == 1 && p.f[0] == aff(0, 3, E));   // folded into the first column factor
        CHECK(norm(v, prog({COL(E), K(2, 0), K(1, 1), ADD, MUL}), &p) && p.scale == 3 && p.f[0] == aff(0, 21, E));
        CHECK(!norm(v, prog({COL(E), COL(D), ADD}), &p));                      // col + col
        CHECK(!norm(v, prog({K(INT64_MAX, 0), K(2, 0), MUL, COL(E), MUL}), &p));   // the constant fold overflows
        CHECK(!norm(v, prog({K(INT64_MAX, 0), COL(D), ADD}), &p));             // aligning the constant to scale 2 overflows
        CHECK(!norm(v, prog({COL(NQ)}), &p));                                  // NULL-able
        CHECK(!norm(v, prog({COL(K0)}), &p) && !norm(v, prog({COL(NCOLS)}), &p) && !norm(v, prog({K(1, 0)}), &p) && !norm(v, prog({COL(E), MUL}), &p));
    }
    // ---- the 24-bit factor bound
    for (int64_t s : {1, -1}) {
        int32_t Ac = 0, Bc = 0;
        CHECK(factor24(aff(100, s * ((1 << 23) - 1), 0), 3, &Ac, &Bc) && Bc == s * ((1 << 23) - 1) && Ac == 100 + 3 * s * ((1 << 23) - 1));
        CHECK(!factor24(aff(100, s * (1 << 23), 0), 3, &Ac, &Bc));
    }
    // ---- a value interval over the codes of [min, max] = [100, 355]
    {
        uint32_t lo, hi;
        code_bounds(100, 355, 0, 99, &lo, &hi); CHECK(lo > hi);                          // below
        code_bounds(100, 355, 356, 1000, &lo, &hi); CHECK(lo > hi);                      // above
        code_bounds(100, 355, 50, 120, &lo, &hi); CHECK(lo == 0 && hi == 20);            // straddling min
        code_bounds(100, 355, 300, INT64_MAX, &lo, &hi); CHECK(lo == 200 && hi == 255);  // straddling max
        code_bounds(100, 355, INT64_MIN, INT64_MAX, &lo, &hi); CHECK(lo == 0 && hi == 255);
        code_bounds(100, 355, 101, 354, &lo, &hi); CHECK(lo == 1 && hi == 254);          // inside
        code_bounds(100, 355, 200, 199, &lo, &hi); CHECK(lo > hi);                       // empty
        code_bounds(INT64_MIN, INT64_MIN + 0xffffffffll, INT64_MIN + 1, INT64_MAX, &lo, &hi); CHECK(lo == 1 && hi == 0xffffffffu);
    }
    // ---- the roles of lowcard_chain
    Range ship; ship.col = SHIP; ship.hi = 10449;
    Range qty; qty.col = QTY; qty.hi = 23;
    const std::vector<ph_rpn> q = prog({COL(QTY)}), e = prog({COL(E)}), d = prog({COL(D)}), star;
    {
        Roles r = roles(v, {q, e, dp, charge, d, star}, {ship});   // Q1
        CHECK(accs(r, {0, 1, 2, 3, 4, 5}) && r.R.p == SHIP && r.R.q == QTY && r.R.e == E && r.R.d == D && r.R.t == T);
        CHECK(r.R.f1 == aff(100, -1, D) && r.R.f2 == aff(100, 1, T) && r.R.aggs[3].scale == 6 && r.R.aggs[2].scale == 4);
        r = roles(v, {star, d, charge, dp, e, q}, {ship});         // reversed
        CHECK(accs(r, {5, 4, 3, 2, 1, 0}) && r.R.e == E && r.R.d == D && r.R.t == T);
        r = roles(v, {q, e, dp, d, star}, {ship});                 // no tax chain
        CHECK(accs(r, {0, 1, 2, 4, 5}) && r.R.t == -1 && r.R.have_f1 && !r.R.have_f2);
        fill_standins(&r.R);
        CHECK(r.R.t == E && r.R.f2 == aff(1, 0, E) && r.R.f1 == aff(100, -1, D));
        r = roles(v, {e, dp, charge, d, star}, {ship});            // no SUM(quantity)
        CHECK(accs(r, {1, 2, 3, 4, 5}) && r.R.q == -1);
        fill_standins(&r.R);
        CHECK(r.R.q == SHIP);
        r = roles(v, {e, d}, {ship});                              // singles: the first 64-bit single is e
        CHECK(accs(r, {1, 4}) && r.R.e == E && r.R.d == D && r.R.q == -1 && r.R.t == -1 && !r.R.have_f1);
        fill_standins(&r.R);
        CHECK(r.R.t == E && r.R.q == SHIP && r.R.f1 == aff(1, 0, D) && r.R.f2 == aff(1, 0, E));
        r = roles(v, {d, e}, {ship});                              // SUM(d) listed first plays e
        CHECK(accs(r, {1, 4}) && r.R.e == D && r.R.d == E);
        for (int s : {6, 7}) {                                     // f1 = (5 10^s + 3) - 10^s d5: the multiplier on either side of 2^23
            int64_t m = 1; for (int i = 0; i < s; i++) m *= 10;
            std::vector<ph_rpn> dp5 = prog({COL(E), K(5 * m + 3, s), COL(D5), SUB, MUL}), ch5 = dp5;
            for (ph_rpn o : {K(1, 0), COL(T), ADD, MUL}) ch5.push_back(o);
            r = roles(v, {q, e, dp5, ch5, prog({COL(D5)}), star}, {ship});
            int32_t Ac = 0, Bc = 0;
            CHECK(accs(r, {0, 1, 2, 3, 4, 5}) && r.R.d == D5 && r.R.f1 == aff(5 * m + 3, -m, D5) && r.R.aggs[2].scale == 2 + s);
            CHECK(affine_bound(r.R.f1, 5, 5) == 3.0L && factor24(r.R.f1, 5, &Ac, &Bc) == (s == 6) && (s != 6 || (Ac == 3 && Bc == -m)));
        }
        r = roles(v, {e, e, star}, {ship});
        CHECK(accs(r, {1, 1, 5}));
        r = roles(v, {e, d, prog({COL(T)})}, {ship});              // a third 64-bit single has no accumulator
        CHECK(r.rc == ROLES_NO_MATCH);
        r = roles(v, {prog({K(1, 0), COL(D), SUB, COL(E), MUL, K(1, 0), COL(T), ADD, MUL}), star}, {ship});   // (1 - d) e (1 + t)
        CHECK(r.rc == ROLES_NO_MATCH);
        r = roles(v, {dp, prog({COL(E), K(1, 0), COL(T), SUB, MUL})}, {ship});   // two different chains
        CHECK(r.rc == ROLES_NO_MATCH);
        r = roles(v, {q, prog({COL(I2)})}, {ship});                // two int32 sums
        CHECK(r.rc == ROLES_NO_MATCH);
        r = roles(v, {q, e, dp, charge, d, star}, {ship, qty});
        CHECK(r.rc == ROLES_NEED_ONE_RANGE);
        r = roles(v, {q, e}, {});
        CHECK(r.rc == ROLES_NEED_ONE_RANGE);
        Range onE; onE.col = E;
        r = roles(v, {q, e}, {onE});
        CHECK(r.rc == ROLES_NEED_ONE_RANGE);
        r = roles(v, {q, star}, {ship});
        CHECK(r.rc == ROLES_NO_SUM64);
    }
    if (!fails) std::printf("scan_lower ok\n");
    return fails ? 1 : 0;
}
"""


def test_scan_lower_on_the_host(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the host-only check of scan_lower.h needs a C++17 host compiler")
    src = tmp_path / "scan_lower_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "scan_lower_check"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'plan_amd' / 'csrc'}", f"-I{ROOT / 'include'}",
                         str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "scan_lower ok"
