// Lowering of a scan descriptor (predicates, aggregate programs) to what the fused scans compute: integer ranges per column, products of
// affine column factors, the roles of the lowcard_chain kernel. Plain host arithmetic over a few facts per column (ColView), with no HIP
// in it: scan_plan.hip fills the views from a ph_table, tests/test_scan_lower.py runs the same functions from a g++ program.
//
// What is normalised here are the reference's plan-time typing rules, because they decide which
// integer kernel an SQL operator becomes:
//  * a DECIMAL column compared with a FLOAT literal is compared as float32 after
//    decimal -> float64 -> float32 (bindAConst builder_binder.go:264-273, MaxLType ltype.go:626-643,
//    tryCastDecimalToFloat32 function_cast.go:349-354). That cast is monotone in the unscaled
//    integer, so the predicate is lowered on the host to an integer threshold found by bisection
//    with the exact cast; the device compares integers.
//  * `<` on FLOAT, `=`/`<`/`<=`/`>=` on DECIMAL, `=` on BIGINT ... have no implementation in
//    selectOperation (function_operator_boolean.go:393-504) and select nothing.
//  * decimal Mul adds scales, Add/Sub takes the max (function_scalar.go:37-84, 429-475); integer
//    literals enter at scale 0 (tryCastInt32ToDecimal function_cast.go:337-347).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "planhip.h"

namespace ph {

// what the lowering reads of a table column
struct ColView {
    int32_t type = 0, scale = 0;
    bool nullable = false, has_range = false;
    int64_t min = 0, max = 0;
    const std::vector<std::string> *dict = nullptr;   // PH_CODE8
};

struct Affine {  // A + B * col   (col < 0: constant A)
    int64_t A = 0, B = 0;
    int32_t col = -1;
    bool operator==(const Affine &o) const { return A == o.A && B == o.B && col == o.col; }
    bool pure() const { return A == 0 && B == 1 && col >= 0; }
};

struct Prod {  // product of factors at `scale` fractional digits
    std::vector<Affine> f;
    int32_t scale = 0;
    bool operator==(const Prod &o) const { return f == o.f && scale == o.scale; }
};

inline bool mul_ok(int64_t a, int64_t b, int64_t *out) { return !__builtin_mul_overflow(a, b, out); }

inline bool pow10_i64(int k, int64_t *out) {
    int64_t r = 1;
    for (int i = 0; i < k; i++)
        if (!mul_ok(r, 10, &r)) return false;
    *out = r;
    return true;
}

inline bool is_i32(const ColView &c) { return c.type == PH_I32 || c.type == PH_DATE; }
inline bool is_i64(const ColView &c) { return c.type == PH_I64 || c.type == PH_DEC64; }

// RPN -> product of affine factors; false = shape outside the fused kernels
inline bool normalize(const ColView *cols, int32_t ncols, const ph_rpn *prog, int32_t n, Prod *out) {
    std::vector<Prod> st;
    for (int32_t i = 0; i < n; i++) {
        const ph_rpn &o = prog[i];
        switch (o.op) {
        case PH_X_COL: {
            if (o.col < 0 || o.col >= ncols) return false;
            const ColView &c = cols[o.col];
            if (c.nullable) return false;  // NULL-able inputs take the generic path
            Prod p;
            Affine a;
            a.B = 1;
            a.col = o.col;
            if (c.type == PH_DEC64) p.scale = c.scale;
            else if (c.type == PH_I32 || c.type == PH_I64) p.scale = 0;
            else return false;
            p.f.push_back(a);
            st.push_back(p);
            break;
        }
        case PH_X_CONST: {
            Prod p;
            Affine a;
            a.A = o.ival;
            p.scale = o.scale;
            p.f.push_back(a);
            st.push_back(p);
            break;
        }
        case PH_X_ADD: case PH_X_SUB: {
            if (st.size() < 2) return false;
            Prod y = st.back(); st.pop_back();
            Prod x = st.back(); st.pop_back();
            if (x.f.size() != 1 || y.f.size() != 1) return false;
            Affine a = x.f[0], b = y.f[0];
            if (a.col >= 0 && b.col >= 0) return false;
            int32_t s = std::max(x.scale, y.scale);
            int64_t mx, my;
            if (!pow10_i64(s - x.scale, &mx) || !pow10_i64(s - y.scale, &my)) return false;
            if (!mul_ok(a.A, mx, &a.A) || !mul_ok(a.B, mx, &a.B) || !mul_ok(b.A, my, &b.A) ||
                !mul_ok(b.B, my, &b.B)) return false;
            if (o.op == PH_X_SUB) { b.A = -b.A; b.B = -b.B; }
            Affine r;
            if (__builtin_add_overflow(a.A, b.A, &r.A)) return false;
            r.B = a.col >= 0 ? a.B : b.B;
            r.col = a.col >= 0 ? a.col : b.col;
            Prod p;
            p.scale = s;
            p.f.push_back(r);
            st.push_back(p);
            break;
        }
        case PH_X_MUL: {
            if (st.size() < 2) return false;
            Prod y = st.back(); st.pop_back();
            Prod x = st.back(); st.pop_back();
            x.f.insert(x.f.end(), y.f.begin(), y.f.end());
            x.scale += y.scale;
            st.push_back(x);
            break;
        }
        default: return false;
        }
    }
    if (st.size() != 1) return false;
    // fold constant factors into the first column factor
    Prod p = st[0];
    int64_t k = 1;
    std::vector<Affine> cols_f;
    for (auto &a : p.f) {
        if (a.col < 0) { if (!mul_ok(k, a.A, &k)) return false; }
        else cols_f.push_back(a);
    }
    if (cols_f.empty()) return false;
    if (!mul_ok(cols_f[0].A, k, &cols_f[0].A) || !mul_ok(cols_f[0].B, k, &cols_f[0].B)) return false;
    p.f = cols_f;
    *out = p;
    return true;
}

// inclusive integer range a predicate restricts a column to; never = selects nothing
struct Range {
    int32_t col = -1;
    int64_t lo = INT64_MIN, hi = INT64_MAX;
    bool never = false;
};

inline float dec_to_f32(int64_t d, int scale) {  // tryCastDecimalToFloat32 for |d| < 2^53
    double p = 1;
    for (int i = 0; i < scale; i++) p *= 10;
    return (float)((double)d / p);
}

// smallest d in [lo,hi] with pred(d) true, for a monotone (false..true) predicate; hi+1 if none
template <typename F> int64_t first_true(int64_t lo, int64_t hi, F pred) {
    if (!pred(hi)) return hi == INT64_MAX ? hi : hi + 1;
    while (lo < hi) {
        int64_t mid = lo + (hi - lo) / 2;
        if (pred(mid)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// column `op` k as a range (op one of PH_EQ .. PH_GE, PH_NE excluded by the callers)
inline void range_of(int32_t op, int64_t k, Range *r) {
    switch (op) {
    case PH_EQ: r->lo = r->hi = k; break;
    case PH_LT: if (k == INT64_MIN) r->never = true; else r->hi = k - 1; break;
    case PH_LE: r->hi = k; break;
    case PH_GT: if (k == INT64_MAX) r->never = true; else r->lo = k + 1; break;
    case PH_GE: r->lo = k; break;
    default: break;
    }
}

// predicate p over its column c -> *r. PH_EUNSUPPORTED: not a range (the caller's next shape, or the generic path)
inline int lower_pred(const ColView &c, const ph_pred &p, Range *r) {
    if (c.nullable) return PH_EUNSUPPORTED;
    r->col = p.col;
    const int32_t op = p.op;
    auto range_from = [&](int64_t k) { range_of(op, k, r); };
    switch (c.type) {
    case PH_I32:
        if (p.k.type != PH_I32) return PH_EUNSUPPORTED;
        if (op == PH_NE) return PH_EUNSUPPORTED;  // not a range: generic path
        if (op < PH_EQ || op > PH_GE) { r->never = true; return PH_OK; }
        range_from((int32_t)p.k.i);
        return PH_OK;
    case PH_DATE:
        if (p.k.type != PH_DATE) return PH_EUNSUPPORTED;
        if (op == PH_EQ || op == PH_NE || op < PH_EQ || op > PH_GE) { r->never = true; return PH_OK; }  // no DATE '='
        range_from((int32_t)p.k.i);
        return PH_OK;
    case PH_I64:
        r->never = true;  // no BIGINT comparison is implemented in selectOperation
        return PH_OK;
    case PH_CODE8: {
        if (p.k.type != PH_STR || !p.k.s) return PH_EUNSUPPORTED;
        if (op != PH_EQ) return PH_EUNSUPPORTED;
        int code = -1;
        for (size_t i = 0; c.dict && i < c.dict->size(); i++)
            if ((*c.dict)[i] == p.k.s) code = (int)i;
        if (code < 0) r->never = true; else r->lo = r->hi = code;
        return PH_OK;
    }
    case PH_DEC64: {
        if (p.k.type == PH_F32) {
            // float32 comparison: >, >=, <= exist; <, =, != do not (FLOAT rows of selectOperation)
            if (op != PH_GT && op != PH_GE && op != PH_LE) { r->never = true; return PH_OK; }
            if (!c.has_range) return PH_EUNSUPPORTED;
            const int64_t LIM = 1ll << 53;
            if (c.min <= -LIM || c.max >= LIM) return PH_EUNSUPPORTED;
            float kf = (float)p.k.f;
            int sc = c.scale;
            int64_t lo = c.min, hi = c.max;
            if (op == PH_GE) {
                int64_t d = first_true(lo, hi, [&](int64_t x) { return dec_to_f32(x, sc) >= kf; });
                if (d > hi) r->never = true; else r->lo = d;
            } else if (op == PH_GT) {
                int64_t d = first_true(lo, hi, [&](int64_t x) { return dec_to_f32(x, sc) > kf; });
                if (d > hi) r->never = true; else r->lo = d;
            } else {  // LE: everything below the first value that is > kf
                int64_t d = first_true(lo, hi, [&](int64_t x) { return dec_to_f32(x, sc) > kf; });
                if (d == lo && dec_to_f32(lo, sc) > kf) r->never = true; else r->hi = d > hi ? hi : d - 1;
            }
            return PH_OK;
        }
        if (p.k.type == PH_DEC64) {
            if (op != PH_GT) { r->never = true; return PH_OK; }  // only DECIMAL '>' exists
            // align the literal to the column scale (exact when the literal has fewer digits)
            if (p.k.scale > c.scale) return PH_EUNSUPPORTED;
            int64_t m, k;
            if (!pow10_i64(c.scale - p.k.scale, &m) || !mul_ok(p.k.i, m, &k)) return PH_EUNSUPPORTED;
            range_from(k);
            return PH_OK;
        }
        return PH_EUNSUPPORTED;
    }
    default:
        return PH_EUNSUPPORTED;
    }
}

// a conjunct's range into the one range kept per column (in the order the columns first appear)
inline void merge_range(std::vector<Range> &ranges, const Range &r) {
    for (auto &q : ranges)
        if (q.col == r.col) {
            q.lo = std::max(q.lo, r.lo);
            q.hi = std::min(q.hi, r.hi);
            q.never |= r.never;
            return;
        }
    ranges.push_back(r);
}

// some conjunct, or the intersection of a column's conjuncts, selects nothing
inline bool selects_nothing(const std::vector<Range> &ranges) {
    for (auto &q : ranges)
        if (q.never || q.lo > q.hi) return true;
    return false;
}

inline int32_t clamp32(int64_t v) { return (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, v)); }

// |A + B*x| over x in [mn,mx], as a long double bound
inline long double affine_bound(const Affine &a, int64_t mn, int64_t mx) {
    long double v1 = (long double)a.A + (long double)a.B * (long double)mn;
    long double v2 = (long double)a.A + (long double)a.B * (long double)mx;
    return std::max(fabsl(v1), fabsl(v2));
}
inline long double value_bound(const ColView &c) { return std::max(fabsl((long double)c.min), fabsl((long double)c.max)); }

// [lo, hi] over the values of a column with statistics [mn, mx] -> over the codes of its narrowed copy (value - mn): a bound below mn
// selects from code 0, one above mx up to the last code, an interval outside [mn, mx] or empty selects nothing (lo 1 > hi 0)
inline void code_bounds(int64_t mn, int64_t mx, int64_t lo, int64_t hi, uint32_t *clo, uint32_t *chi) {
    lo = std::max(lo, mn);
    hi = std::min(hi, mx);
    if (lo > hi) {
        *clo = 1;
        *chi = 0;
        return;
    }
    *clo = (uint32_t)((uint64_t)lo - (uint64_t)mn);   // < 2^32: the copy exists only when mx - mn does
    *chi = (uint32_t)((uint64_t)hi - (uint64_t)mn);
}

// f = A + B (base + code) = Ac + Bc code, to be one v_mad_i32_i24 on a one-byte code: Bc inside the signed 24-bit operand range (the
// instruction ignores operand bits above 24, so a B outside it would give wrong sums, not an error). Ac = f at code 0 fits 32 bits because
// |f| < 2^31 over the column (the caller's bound).
inline bool factor24(const Affine &f, int64_t base, int32_t *Ac, int32_t *Bc) {
    constexpr int64_t I24_MAX = (1 << 23) - 1;
    if (f.B < -I24_MAX || f.B > I24_MAX) return false;
    *Ac = (int32_t)(int64_t)((__int128)f.A + (__int128)f.B * base);
    *Bc = (int32_t)f.B;
    return true;
}

// ---------------------------------------------------------------- lowcard_chain: which column plays which role

// a requested aggregate: its kind and, unless it is COUNT(*), its normalised argument
struct AggReq {
    int32_t kind = 0;
    Prod p;
    bool star = false;
};

// requested aggregate -> the accumulator word that holds it
struct AggMap { int32_t kind; int acc; int32_t scale; };

// The kernel's accumulators are Σq, Σe, Σe·f1, Σe·f1·f2, Σd, count with f1 = A1 + B1 d, f2 = A2 + B2 t over an int32 column q and 64-bit
// columns e, d, t, behind one range predicate on an int32 column p. q, d, t = -1: the plan names no column for the role.
struct LowcardRoles {
    int32_t p = -1, q = -1, e = -1, d = -1, t = -1;
    Affine f1, f2;
    bool have_f1 = false, have_f2 = false;
    std::vector<AggMap> aggs;   // by request
};

enum RolesResult { ROLES_OK = 0, ROLES_NO_MATCH, ROLES_NEED_ONE_RANGE, ROLES_NO_SUM64 };

// The requests are matched longest chain first, so that the chains name e, d and t before the single columns are told apart: a 64-bit
// single is Σe when it is e (or the first single of a plan without a chain), Σd when it is d (or d is still free).
inline RolesResult match_lowcard_roles(const std::vector<AggReq> &reqs, const std::vector<Range> &ranges, const ColView *cols, LowcardRoles *out) {
    LowcardRoles R;
    if (ranges.size() != 1 || !is_i32(cols[ranges[0].col])) return ROLES_NEED_ONE_RANGE;
    R.p = ranges[0].col;
    std::vector<size_t> order(reqs.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return reqs[x].p.f.size() > reqs[y].p.f.size(); });
    R.aggs.resize(reqs.size());
    auto i64 = [&](const Affine &a) { return is_i64(cols[a.col]); };
    for (size_t oi : order) {
        const AggReq &r = reqs[oi];
        AggMap m{r.kind, 5, 0};
        if (!r.star) {
            const std::vector<Affine> &f = r.p.f;
            m.scale = r.p.scale;
            if (f.size() == 3) {
                if (!f[0].pure() || !i64(f[0]) || !i64(f[1]) || !i64(f[2])) return ROLES_NO_MATCH;
                if (R.have_f2 && !(R.e == f[0].col && R.f1 == f[1] && R.f2 == f[2])) return ROLES_NO_MATCH;
                R.e = f[0].col; R.f1 = f[1]; R.f2 = f[2]; R.have_f1 = R.have_f2 = true;
                R.d = R.f1.col; R.t = R.f2.col;
                m.acc = 3;
            } else if (f.size() == 2) {
                if (!f[0].pure() || !i64(f[0]) || !i64(f[1])) return ROLES_NO_MATCH;
                if (R.have_f1 && !(R.e == f[0].col && R.f1 == f[1])) return ROLES_NO_MATCH;
                R.e = f[0].col; R.f1 = f[1]; R.have_f1 = true; R.d = R.f1.col;
                m.acc = 2;
            } else if (f.size() == 1 && f[0].pure()) {
                const int32_t c = f[0].col;
                if (is_i32(cols[c])) { if (R.q >= 0 && R.q != c) return ROLES_NO_MATCH; R.q = c; m.acc = 0; }
                else if (is_i64(cols[c])) {
                    if (c == R.e || R.e < 0) { R.e = c; m.acc = 1; }
                    else if (c == R.d || R.d < 0) { R.d = c; m.acc = 4; }
                    else return ROLES_NO_MATCH;
                } else return ROLES_NO_MATCH;
            } else return ROLES_NO_MATCH;
        }
        R.aggs[oi] = m;
    }
    if (R.e < 0) return ROLES_NO_SUM64;
    *out = R;
    return ROLES_OK;
}

// the roles a plan does not name read a stand-in (PH_SCAN_JIT=0; otherwise such plans get a generated kernel): e for d and t, p for q, and
// the factor 1 for a chain the plan does not ask for
inline void fill_standins(LowcardRoles *R) {
    if (R->d < 0) R->d = R->e;
    if (R->t < 0) R->t = R->e;
    if (R->q < 0) R->q = R->p;
    if (!R->have_f1) { R->f1 = Affine(); R->f1.A = 1; R->f1.col = R->d; }
    if (!R->have_f2) { R->f2 = Affine(); R->f2.A = 1; R->f2.col = R->t; }
}

}  // namespace ph
