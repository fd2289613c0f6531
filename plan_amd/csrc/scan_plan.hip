// Fused Agg <- Scan(filter) plans: shape matching, overflow proofs, launch sequencing and result assembly for ph_scan_plan_* /
// ph_scan_filter_agg. The descriptor is lowered by scan_lower.h (ranges, products of affine factors, the roles of lowcard_chain), the
// kernel instance of a run is chosen by scan_inst.h; both are plain host arithmetic over column views, checked without a device.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "scan_inst.h"
#include "scan_jit.h"
#include "scan_kernels.h"
#include "scan_lower.h"

namespace {

using ph::set_error;
using ph::Affine;
using ph::AggReq;
using ph::ColView;
using ph::Prod;
using ph::Range;

// one view per table column, filled once per ph_scan_plan_create
std::vector<ColView> col_views(const ph_table *t) {
    std::vector<ColView> v(t->cols.size());
    for (size_t i = 0; i < v.size(); i++) {
        const auto &c = t->cols[i];
        v[i] = ColView{c.type, c.scale, c.validity != nullptr, c.has_range, c.min, c.max, &c.dict};
    }
    return v;
}

bool pred_col_ok(const std::vector<ColView> &cols, const ph_pred &p) {
    if (p.col >= 0 && p.col < (int32_t)cols.size()) return true;
    set_error("predicate column %d out of range", p.col);
    return false;
}

// the narrowed copy of column c (ph_table::column::narrow) as a kernel operand; false = none (or PH_NARROW=0)
bool for_col(const ph_table *t, int32_t c, ph::ForCol *f) {
    const auto &d = t->cols[(size_t)c];
    if (!ph::narrow_enabled() || !d.narrow) return false;
    f->data = (const uint8_t *)d.narrow;
    f->base = d.min;
    f->w = d.narrow_w;
    return true;
}

// ---- the switches, one reader per time of reading
bool env_is(const char *name, char c) {
    const char *e = getenv(name);
    return e && e[0] == c;
}

// once per process. PH_SCAN_LEAN=0: plans never take the lean instances of the narrow kernels, so every plan runs the kernel it ran before them
// (A/B runs, and the bit-for-bit comparison of the tests); PH_SCAN_TAIL=0: merge kernel, then publish_kernel at the fetch
const ph::ScanSwitches &process_switches() {
    static const ph::ScanSwitches s = [] {
        ph::ScanSwitches v;
        v.nt = !env_is("PH_SCAN_NT", '0');
        v.narrow_generic = env_is("PH_SCAN_NARROW_GENERIC", '1');
        v.pack_generic = env_is("PH_SCAN_PACK_GENERIC", '1');
        v.lean = !env_is("PH_SCAN_LEAN", '0');
        v.tail = !env_is("PH_SCAN_TAIL", '0');
        return v;
    }();
    return s;
}

// at every create. PH_SCAN_JIT=1: prefer the plan-specialised kernel even for the two precompiled shapes (A/B); PH_SCAN_JIT=0: never
// generate code; -1: not set
int jit_switch() {
    const char *je = getenv("PH_SCAN_JIT");
    return je ? atoi(je) : -1;
}

// PH_SCAN_HIST=0 (at every run and every ph_scan_plan_row_body, so one process can run both bodies): the columns body
bool hist_switch() { return !env_is("PH_SCAN_HIST", '0'); }

}  // namespace

enum PlanKind { PK_FILTER_SUMPROD = 1, PK_LOWCARD_CHAIN = 2, PK_GENERIC = 3, PK_JIT = 4 };

struct ph_scan_plan {
    ph_ctx *ctx = nullptr;
    const ph_table *t = nullptr;
    int kind = 0;
    bool never = false;  // some conjunct selects nothing
    ph::FilterSumProdParams fs{};
    ph::LowcardChainParams lc{};
    int32_t lc_cols[7] = {-1, -1, -1, -1, -1, -1, -1};   // PK_LOWCARD_CHAIN: the table columns of p, q, e, d, t, k0, k1 (the key of the packed scan group)
    int max_grid = 0;
    int nacc = 0;  // accumulators per launch (nslots * LC_NACC, or 2)
    // requested aggregates -> accumulator
    using AggMap = ph::AggMap;
    std::vector<AggMap> aggs;
    int32_t nkeys = 0;
    int32_t group_cols[4] = {-1, -1, -1, -1};
    // layout of the raw accumulator words of the fused kinds: per group slot `stride` words, the
    // count at cnt_idx, the first-seen row id at first_idx (-1: none), ops[j] = how word j merges
    // (0 sum, 1 min, 2 max); slot = dense index over gcard
    int nslots = 1, stride = 0, cnt_idx = 0, first_idx = -1;
    std::vector<int> ops, gcard;
    // PK_JIT: the plan-specialised kernel
    ph::JitShape jshape;
    ph::JitKernel jkernel;
    ph::JitParams jparams{};
    // device buffers
    long long *partials = nullptr;
    unsigned long long *out_lo = nullptr;
    long long *out_hi = nullptr;
    long double row_bound = 0;  // largest |per-row accumulator value|
    int32_t bytes_per_row = 0;  // bytes per row the scan kernel loads (ph_scan_plan_bytes_per_row)
    int64_t last_rows = 0;
    int last_grid = 0;
    int last_inst = -1;      // PK_LOWCARD_CHAIN: the LcInst of the last run, -1 before the first (ph_scan_plan_row_body)
    unsigned long long armed_seq = 0;   // the last run's own publish (ScanTail), 0 = none: fetch downloads
    bool unfetched = false;             // the last run's result was never fetched: a caller that runs back to back (a throughput loop, the N-rank
                                        // path reading the partials on the device) gets no publish armed — the mailbox store is a system fence per run
    // PK_GENERIC: the descriptor itself, run through the operator-granular kernels
    std::vector<ph_pred> g_preds;
    std::vector<std::string> g_pred_strs;
    std::vector<int32_t> g_groups;
    std::vector<ph_aggexpr> g_aggs;
    ph_agg *g_agg = nullptr;
};

// workgroups `partials` holds: the plan's own grid, or what PH_SCAN_GRID and the bins body's tile bound may raise it to
static int partials_cap(const ph_scan_plan *p) { return std::max(p->max_grid, 8192); }

// The plan's two device buffers come from the ctx's stream-ordered pool: a plan that is created, run, fetched and freed per query — the
// executor behind the operator interface is built and closed per query, like the reference's — then costs no hipMalloc / hipFree. Both
// synchronise the device: rocprofv3 --hip-trace of Q1 at SF10 behind OperatorExec showed two hipFree calls of ~160 us each per query,
// the whole of the 0.28 ms it stood above the fused kernel (profiles/r04_q1_opif_before_hip_api_stats.csv).
static int plan_alloc(ph_scan_plan *p) {
    PH_CHECK(p->ctx->pool_alloc((int64_t)partials_cap(p) * p->nacc * (int64_t)sizeof(long long), (void **)&p->partials));
    // one allocation, lo[nacc] then hi[nacc]: the raw partial result other ranks all-gather
    PH_CHECK(p->ctx->pool_alloc((int64_t)p->nacc * 2 * (int64_t)sizeof(unsigned long long), (void **)&p->out_lo));
    p->out_hi = (long long *)(p->out_lo + p->nacc);
    return PH_OK;
}

extern "C" void ph_scan_plan_free(ph_scan_plan *p) {
    if (!p) return;
    // stream-ordered reuse: whatever takes these blocks next is queued behind the plan's last kernel on the ctx's one stream
    if (p->partials) p->ctx->pool_release(p->partials);
    if (p->out_lo) p->ctx->pool_release(p->out_lo);
    if (p->g_agg) ph_agg_free(p->g_agg);
    delete p;
}

// ---------------------------------------------------------------- the instance a plan launches (scan_inst.h)

static ph::FsFacts fs_facts(const ph::FilterSumProdParams &P) { return ph::FsFacts{P.form, {P.np0.w, P.np2.w, P.nb.w, P.na.w}}; }

// tiles_fit: the run's tiles per workgroup are within the bins body's bound (scan_geometry)
static ph::LcFacts lc_facts(const ph::LowcardChainParams &P, bool tiles_fit) {
    const bool group = P.pk != nullptr;
    return ph::LcFacts{P.form, {P.np.w, P.nq.w, P.ne.w, P.nd.w, P.nt.w}, P.lean != 0, group, group && ph::is_lineitem_layout(P.pk_shift, P.pk_width),
                       P.nslots, tiles_fit, group && P.pk_form == ph::SG_SPLIT56};
}

extern "C" const char *ph_scan_plan_kind(const ph_scan_plan *p) {
    if (!p) return "";
    return p->kind == PK_FILTER_SUMPROD ? "filter_sumprod" : p->kind == PK_LOWCARD_CHAIN ? "lowcard_chain" : p->kind == PK_JIT ? "jit" : "generic";
}

extern "C" int32_t ph_scan_plan_bytes_per_row(const ph_scan_plan *p) { return p ? p->bytes_per_row : 0; }

extern "C" const char *ph_scan_plan_variant(const ph_scan_plan *p) {
    if (!p) return "";
    if (p->kind == PK_FILTER_SUMPROD) return ph::fs_variant_name(ph::fs_choose(fs_facts(p->fs), process_switches()));
    if (p->kind == PK_LOWCARD_CHAIN) return ph::lc_variant_name(ph::lc_choose(lc_facts(p->lc, true), process_switches()));
    return ph_scan_plan_kind(p);
}

// the row body of the plan's next launch: the bins body unless the last run's tiles did not fit it (or PH_SCAN_HIST=0 held then, or holds now)
extern "C" const char *ph_scan_plan_row_body(const ph_scan_plan *p) {
    if (!p || p->kind != PK_LOWCARD_CHAIN || !(p->last_inst < 0 || ph::lc_takes_bins((ph::LcInst)p->last_inst))) return "columns";
    ph::ScanSwitches sw = process_switches();
    sw.hist = hist_switch();
    return ph::lc_row_body_name(ph::lc_choose(lc_facts(p->lc, true), sw));
}

// ---------------------------------------------------------------- the two precompiled shapes

// filter_sumprod: SUM(a*b) [+ COUNT(*)], ranges on <=2 int32 + <=1 int64 col
static int plan_filter_sumprod(ph_ctx *ctx, const ph_table *t, const std::vector<ColView> &cols, const std::vector<Range> &ranges,
                               const std::vector<AggReq> &reqs, ph_scan_plan *p) {
    p->kind = PK_FILTER_SUMPROD;
    // ---- the one product: two pure 64-bit column factors
    int32_t a_col = -1, b_col = -1;
    for (size_t i = 0; i < reqs.size(); i++) {
        ph::AggMap m{reqs[i].kind, 1, 0};
        if (!reqs[i].star) {
            const Prod &pr = reqs[i].p;
            if (pr.f.size() != 2 || !pr.f[0].pure() || !pr.f[1].pure() || !is_i64(cols[pr.f[0].col]) || !is_i64(cols[pr.f[1].col])) {
                set_error("aggregate %zu is not SUM(col*col) over 64-bit columns", i);
                return PH_EUNSUPPORTED;
            }
            if (a_col >= 0 && !(a_col == pr.f[0].col && b_col == pr.f[1].col)) return PH_EUNSUPPORTED;
            a_col = pr.f[0].col;
            b_col = pr.f[1].col;
            m.acc = 0;
            m.scale = pr.scale;
        }
        p->aggs.push_back(m);
    }
    if (a_col < 0) { set_error("filter_sumprod needs one SUM(col*col)"); return PH_EUNSUPPORTED; }
    // ---- the predicate columns
    std::vector<Range> r32, r64;
    for (auto &r : ranges) (is_i32(cols[r.col]) ? r32 : r64).push_back(r);
    for (auto &r : ranges) if (!is_i32(cols[r.col]) && !is_i64(cols[r.col])) return PH_EUNSUPPORTED;
    if (r32.empty() || r32.size() > 2 || r64.size() > 1) { set_error("filter_sumprod: predicate columns do not fit (need 1-2 int32, 0-1 int64)"); return PH_EUNSUPPORTED; }
    ph::FilterSumProdParams &F = p->fs;
    F.b_lo = INT64_MIN;
    F.b_hi = INT64_MAX;
    if (!r64.empty()) {
        // the 64-bit predicate column must be one of the factors; make it `b`
        if (r64[0].col == a_col) std::swap(a_col, b_col);
        if (r64[0].col != b_col) return PH_EUNSUPPORTED;
        F.b_lo = r64[0].lo;
        F.b_hi = r64[0].hi;
    }
    const Range &first = r32[0], &second = r32.size() > 1 ? r32[1] : r32[0];
    auto data = [&](int32_t c) { return t->cols[(size_t)c].data; };
    F.p0 = (const int32_t *)data(first.col);
    F.p0_lo = ph::clamp32(first.lo);
    F.p0_hi = ph::clamp32(first.hi);
    F.p2 = (const int32_t *)data(second.col);
    F.p2_lo = ph::clamp32(second.lo);
    F.p2_hi = ph::clamp32(second.hi);
    F.a = (const int64_t *)data(a_col);
    F.b = (const int64_t *)data(b_col);
    // ---- the overflow bound of a row
    if (!cols[a_col].has_range || !cols[b_col].has_range) return PH_EUNSUPPORTED;
    const long double ba = ph::value_bound(cols[a_col]), bb = ph::value_bound(cols[b_col]);
    p->row_bound = ba * bb;
    p->bytes_per_row = ph::type_width(cols[first.col].type) + ph::type_width(cols[second.col].type) + 16;
    // ---- the narrowed copies when all four columns have one: 16 rows per lane, predicates over codes, a and b decoded to int64
    if (for_col(t, first.col, &F.np0) && for_col(t, second.col, &F.np2) && for_col(t, b_col, &F.nb) && for_col(t, a_col, &F.na)) {
        ph::code_bounds(cols[first.col].min, cols[first.col].max, first.lo, first.hi, &F.np0_lo, &F.np0_hi);
        ph::code_bounds(cols[second.col].min, cols[second.col].max, second.lo, second.hi, &F.np2_lo, &F.np2_hi);
        ph::code_bounds(cols[b_col].min, cols[b_col].max, F.b_lo, F.b_hi, &F.nb_lo, &F.nb_hi);
        const long double LIM32 = 2147483647.0L;
        F.form = ba <= LIM32 && bb <= LIM32 ? ph::FORM_NARROW32 : ph::FORM_NARROW;
        p->bytes_per_row = F.np0.w + F.np2.w + F.nb.w + F.na.w;
    }
    p->nacc = 2;
    p->nslots = 1; p->stride = 2; p->cnt_idx = 1; p->first_idx = -1; p->ops = {0, 0};
    // ---- the grid
    // one 256-thread workgroup per CU (1 wave per SIMD) streams fastest: measured on MI355X,
    // SF10: 6.48 TB/s at grid 256 vs 5.95 at 2048 and 4.6-5.4 at grids that are not a
    // multiple of the CU count (tail imbalance); scripts/ab_scan2.sh
    p->max_grid = ctx->cu_count;
    // the narrow kernel issues 16 rows per lane and tile: with one wave per SIMD it is bound by instruction issue (SQ_ACTIVE_INST_ANY
    // 67 % of SQ_WAVE_CYCLES in Q1's form); two workgroups per CU hide it (SF10: Q6 0.158 -> 0.107 ms per step)
    if (F.form != ph::FORM_WIDE) p->max_grid = 2 * ctx->cu_count;
    return PH_OK;
}

// lowcard_chain, step 2: the columns of the matched roles into the kernel's parameters — pointers, the per-row overflow bound, and the
// narrowed copies with the form (32-bit products, lean factors) their value ranges prove
static int bind_lowcard_columns(const ph_table *t, const std::vector<ColView> &cols, const Range &range, const ph::LowcardRoles &R, ph_scan_plan *p) {
    ph::LowcardChainParams &C = p->lc;
    auto data = [&](int32_t c) { return t->cols[(size_t)c].data; };
    C.p = (const int32_t *)data(R.p);
    C.p_lo = ph::clamp32(range.lo);
    C.p_hi = ph::clamp32(range.hi);
    C.q = (const int32_t *)data(R.q);
    C.e = (const int64_t *)data(R.e);
    C.d = (const int64_t *)data(R.d);
    C.t = (const int64_t *)data(R.t);
    C.A1 = R.f1.A; C.B1 = R.f1.B; C.A2 = R.f2.A; C.B2 = R.f2.B;
    for (int32_t c : {R.q, R.e, R.d, R.t}) if (!cols[c].has_range) return PH_EUNSUPPORTED;
    const long double be = ph::value_bound(cols[R.e]);
    const long double b1 = ph::affine_bound(R.f1, cols[R.d].min, cols[R.d].max);
    const long double b2 = ph::affine_bound(R.f2, cols[R.t].min, cols[R.t].max);
    p->row_bound = std::max({be * b1 * b2, be * b1, be, ph::value_bound(cols[R.d]), ph::value_bound(cols[R.q])});
    p->bytes_per_row = ph::type_width(cols[R.p].type) + ph::type_width(cols[R.q].type) + 3 * 8 + 2;
    // the narrowed copies when all five columns have one (the code columns are read as they are): the overflow proof above is
    // over values, so it holds as it is
    if (for_col(t, R.p, &C.np) && for_col(t, R.q, &C.nq) && for_col(t, R.e, &C.ne) && for_col(t, R.d, &C.nd) && for_col(t, R.t, &C.nt)) {
        ph::code_bounds(cols[R.p].min, cols[R.p].max, range.lo, range.hi, &C.np_lo, &C.np_hi);
        // 32-bit factors: e, f1 = A1 + B1 d, f2 = A2 + B2 t and e f1 all below 2^31 in magnitude (f1, f2 computed modulo 2^32 are then exact)
        const long double LIM32 = 2147483647.0L;
        C.form = be <= LIM32 && b1 <= LIM32 && b2 <= LIM32 && be * b1 <= LIM32 ? ph::FORM_NARROW32 : ph::FORM_NARROW;
        // the lean row body computes f1 and f2 as 24-bit multiply-adds on the (one-byte) codes
        if (C.form == ph::FORM_NARROW32 && process_switches().lean && ph::factor24(R.f1, C.nd.base, &C.A1c, &C.B1c) &&
            ph::factor24(R.f2, C.nt.base, &C.A2c, &C.B2c)) {
            C.lean = 1;
            C.e_base32 = (int32_t)C.ne.base;
        }
        p->bytes_per_row = C.np.w + C.nq.w + C.ne.w + C.nd.w + C.nt.w + 2;
    }
    return PH_OK;
}

// lowcard_chain, step 3: workgroups per CU
static int lowcard_max_grid(const ph_ctx *ctx, const ph::LowcardChainParams &C) {
    // one workgroup per CU: 6.35 TB/s at grid 256 vs 6.0 at 512 (2 per CU is what the
    // per-thread-private LDS accumulators would still allow); scripts/ab_scan2.sh
    // the narrow kernel: two workgroups per CU when their LDS accumulators fit (Q1: 6 slots x 12 KiB each; SF10 0.197 -> 0.154 ms
    // per step, the same issue bound as filter_sumprod's)
    const int64_t lds = (int64_t)C.nslots * (5 * 256 * 8 + 2 * 256 * 4);
    return C.form != ph::FORM_WIDE && 2 * lds <= 160 * 1024 ? 2 * ctx->cu_count : ctx->cu_count;
}

// lowcard_chain: two dictionary-code group columns, one int32 range predicate, the accumulators of scan_lower.h's LowcardRoles
static int plan_lowcard_chain(ph_ctx *ctx, const ph_table *t, const std::vector<ColView> &cols, const std::vector<Range> &ranges,
                              const std::vector<AggReq> &reqs, const int32_t *group_cols, int32_t ngroup_cols, bool nojit, ph_scan_plan *p) {
    p->kind = PK_LOWCARD_CHAIN;
    // ---- the group columns: dense slots over two dictionaries
    if (ngroup_cols != 2 || cols[group_cols[0]].type != PH_CODE8 || cols[group_cols[1]].type != PH_CODE8 ||
        cols[group_cols[0]].nullable || cols[group_cols[1]].nullable) {
        set_error("lowcard_chain needs two non-NULL dictionary-code group columns");
        return PH_EUNSUPPORTED;
    }
    int n[2];
    for (int gi = 0; gi < 2; gi++) {
        const ColView &gc = cols[group_cols[gi]];
        n[gi] = gc.dict->empty() ? (int)gc.max + 1 : (int)gc.dict->size();
    }
    // every code must index inside the LDS slots sized from n0*n1: the recorded maxima prove it
    for (int gi = 0; gi < 2; gi++) {
        const ColView &gc = cols[group_cols[gi]];
        if (!gc.has_range || gc.min < 0 || gc.max >= n[gi]) {
            set_error("lowcard_chain: group column %d holds codes outside its dictionary", group_cols[gi]);
            return PH_EUNSUPPORTED;
        }
    }
    if (n[0] * n[1] > ph::LC_MAX_SLOTS || n[0] * n[1] <= 0) { set_error("lowcard_chain: %d group slots exceed %d", n[0] * n[1], ph::LC_MAX_SLOTS); return PH_EUNSUPPORTED; }
    p->nkeys = 2;
    p->group_cols[0] = group_cols[0];
    p->group_cols[1] = group_cols[1];
    // ---- step 1, the roles
    ph::LowcardRoles R;
    switch (ph::match_lowcard_roles(reqs, ranges, cols.data(), &R)) {
    case ph::ROLES_OK: break;
    case ph::ROLES_NEED_ONE_RANGE: set_error("lowcard_chain needs exactly one int32/date range predicate"); return PH_EUNSUPPORTED;
    case ph::ROLES_NO_SUM64: set_error("lowcard_chain needs at least one 64-bit summed column"); return PH_EUNSUPPORTED;
    case ph::ROLES_NO_MATCH: return PH_EUNSUPPORTED;
    }
    p->aggs = R.aggs;
    // The precompiled kernel always loads its four roles; a plan that names fewer columns would
    // re-read a stand-in (measured: 3.5 TB/s of useful bytes instead of 6.3). Such plans get a
    // generated kernel that reads only what they name — unless code generation is switched off.
    if ((R.d < 0 || R.t < 0 || R.q < 0) && !nojit) { set_error("lowcard_chain: the plan names fewer columns than the kernel reads"); return PH_EUNSUPPORTED; }
    ph::fill_standins(&R);
    ph::LowcardChainParams &C = p->lc;
    C.k0 = (const uint8_t *)t->cols[(size_t)group_cols[0]].data;
    C.k1 = (const uint8_t *)t->cols[(size_t)group_cols[1]].data;
    C.nk1 = n[1];
    C.nslots = n[0] * n[1];
    const int32_t roles[7] = {R.p, R.q, R.e, R.d, R.t, group_cols[0], group_cols[1]};
    std::copy(roles, roles + 7, p->lc_cols);
    // ---- step 2, the columns and the form; step 3, the grid
    PH_CHECK(bind_lowcard_columns(t, cols, ranges[0], R, p));
    p->nacc = C.nslots * (ph::LC_NACC + 1);  // + first_row
    p->nslots = C.nslots; p->stride = ph::LC_NACC + 1; p->cnt_idx = 5; p->first_idx = ph::LC_NACC;
    p->ops = {0, 0, 0, 0, 0, 0, 1};
    p->gcard = {n[0], n[1]};
    p->max_grid = lowcard_max_grid(ctx, C);
    return PH_OK;
}

static int try_fused(ph_ctx *ctx, const ph_table *t, const std::vector<ColView> &cols, const ph_pred *preds, int32_t npreds,
                     const int32_t *group_cols, int32_t ngroup_cols, const ph_aggexpr *aggs, int32_t naggs, bool nojit,
                     ph_scan_plan **out) {
    // ---- predicates -> one range per column
    std::vector<Range> ranges;
    for (int32_t i = 0; i < npreds; i++) {
        if (!pred_col_ok(cols, preds[i])) return PH_EINVAL;
        Range r;
        if (ph::lower_pred(cols[preds[i].col], preds[i], &r) != PH_OK) { set_error("predicate %d is outside the fused shapes", i); return PH_EUNSUPPORTED; }
        ph::merge_range(ranges, r);
    }
    // ---- aggregates -> normalised products
    std::vector<AggReq> reqs;
    for (int32_t a = 0; a < naggs; a++) {
        AggReq r;
        r.kind = aggs[a].kind;
        r.star = aggs[a].kind == PH_A_COUNT_STAR;
        if (!r.star) {
            if (aggs[a].kind != PH_A_SUM && aggs[a].kind != PH_A_AVG && aggs[a].kind != PH_A_COUNT) {
                set_error("aggregate %d: MIN/MAX take the generic path", a);
                return PH_EUNSUPPORTED;
            }
            if (aggs[a].nprog <= 0 || aggs[a].nprog > 12 || !ph::normalize(cols.data(), (int32_t)cols.size(), aggs[a].prog, aggs[a].nprog, &r.p)) {
                set_error("aggregate %d: argument expression is outside the fused shapes", a);
                return PH_EUNSUPPORTED;
            }
        }
        reqs.push_back(r);
    }
    ph_scan_plan *p = new ph_scan_plan();
    p->ctx = ctx;
    p->t = t;
    p->never = ph::selects_nothing(ranges);
    int rc = ngroup_cols == 0 ? plan_filter_sumprod(ctx, t, cols, ranges, reqs, p)
                              : plan_lowcard_chain(ctx, t, cols, ranges, reqs, group_cols, ngroup_cols, nojit, p);
    if (rc == PH_OK) rc = plan_alloc(p);
    if (rc != PH_OK) { ph_scan_plan_free(p); return rc; }
    *out = p;
    return PH_OK;
}

// ---------------------------------------------------------------- plan-specialised (hiprtc) plans
// Any conjunction of range / `!=` predicates over NULL-free fixed-width columns, grouped by up to
// four dictionary-code columns (dense slots that fit the CU's LDS as per-thread-private
// accumulator columns) and aggregated with SUM/AVG/COUNT over products of affine column factors or
// MIN/MAX of a column, becomes one generated kernel (scan_jit.h): only the columns the plan names
// are read, each byte once.
static int try_jit(ph_ctx *ctx, const ph_table *t, const std::vector<ColView> &views, const ph_pred *preds, int32_t npreds,
                   const int32_t *group_cols, int32_t ngroup_cols, const ph_aggexpr *aggs, int32_t naggs,
                   ph_scan_plan **out) {
    auto unsupported = [&](const char *why) { set_error("plan-specialised kernel: %s", why); return PH_EUNSUPPORTED; };
    if (ngroup_cols > 4) return unsupported("more than 4 group columns");
    ph::JitShape S;
    std::vector<long long> consts;
    std::vector<int32_t> tcol;   // loaded column slot -> table column
    auto slot_of = [&](int32_t c) -> int {
        for (size_t i = 0; i < tcol.size(); i++) if (tcol[i] == c) return (int)i;
        const auto &d = t->cols[(size_t)c];
        int w = d.type == PH_CODE8 ? 1 : (d.type == PH_I32 || d.type == PH_DATE) ? 4 : (d.type == PH_I64 || d.type == PH_DEC64) ? 8 : 0;
        if (w == 0 || d.validity) return -1;
        tcol.push_back(c);
        S.col_width.push_back(w);
        return (int)tcol.size() - 1;
    };
    // ---- predicates: one merged range per column, `!=` separately
    std::vector<Range> ranges;
    struct Ne { int32_t col; long long k; };
    std::vector<Ne> nes;
    for (int32_t i = 0; i < npreds; i++) {
        const ph_pred &pr = preds[i];
        if (!pred_col_ok(views, pr)) return PH_EINVAL;
        const ColView &c = views[pr.col];
        if (pr.op == PH_NE && c.type == PH_I32 && pr.k.type == PH_I32 && !c.nullable) { nes.push_back({pr.col, (int32_t)pr.k.i}); continue; }
        Range r;
        if (ph::lower_pred(c, pr, &r) != PH_OK) return unsupported("a predicate does not lower to an integer range");
        ph::merge_range(ranges, r);
    }
    const bool never = ph::selects_nothing(ranges);
    for (auto &q : ranges) {
        int sl = slot_of(q.col);
        if (sl < 0) return unsupported("predicate column type");
        S.preds.push_back({sl, false});
        consts.push_back(q.lo);
        consts.push_back(q.hi);
    }
    for (auto &q : nes) {
        int sl = slot_of(q.col);
        if (sl < 0) return unsupported("predicate column type");
        S.preds.push_back({sl, true});
        consts.push_back(q.k);
    }
    // ---- group columns: dense slot over dictionary codes
    ph_scan_plan *p = new ph_scan_plan();
    p->ctx = ctx; p->t = t; p->kind = PK_JIT; p->never = never;
    auto fail = [&](int rc) { ph_scan_plan_free(p); return rc; };
    int64_t ns = 1;
    for (int32_t g = 0; g < ngroup_cols; g++) {
        int32_t gc = group_cols[g];
        if (gc < 0 || gc >= (int32_t)t->cols.size()) { set_error("group column %d out of range", gc); return fail(PH_EINVAL); }
        const auto &c = t->cols[(size_t)gc];
        if (c.type != PH_CODE8 || c.validity || !c.has_range || c.min < 0) return fail(unsupported("group columns must be NULL-free dictionary codes"));
        int card = (int)std::max<int64_t>((int64_t)c.dict.size(), c.max + 1);
        ns *= card;
        if (ns > 4096) return fail(unsupported("too many group slots"));
        S.group_col.push_back(slot_of(gc));
        S.group_card.push_back(card);
        p->group_cols[g] = gc;
        p->gcard.push_back(card);
    }
    p->nkeys = ngroup_cols;
    S.nslots = (int)ns;
    // ---- aggregates -> deduplicated accumulators
    struct AccReq { int op; Prod pr; };
    std::vector<AccReq> accs;
    long double row_bound = 0;
    for (int32_t a = 0; a < naggs; a++) {
        ph_scan_plan::AggMap m{aggs[a].kind, -1, 0};
        if (aggs[a].kind != PH_A_COUNT_STAR) {
            Prod pr;
            if (aggs[a].nprog <= 0 || aggs[a].nprog > 12 || !ph::normalize(views.data(), (int32_t)views.size(), aggs[a].prog, aggs[a].nprog, &pr)) return fail(unsupported("an aggregate argument is not a product of affine column factors"));
            m.scale = pr.scale;
            int op = aggs[a].kind == PH_A_MIN ? 1 : aggs[a].kind == PH_A_MAX ? 2 : 0;
            if (aggs[a].kind != PH_A_COUNT) {
                if (op != 0 && !(pr.f.size() == 1 && pr.f[0].A == 0 && pr.f[0].B == 1)) return fail(unsupported("MIN/MAX of an expression"));
                if (pr.f.size() > 4) return fail(unsupported("more than 4 factors"));
                int found = -1;
                for (size_t i = 0; i < accs.size(); i++) if (accs[i].op == op && accs[i].pr == pr) found = (int)i;
                if (found < 0) { accs.push_back({op, pr}); found = (int)accs.size() - 1; }
                m.acc = found;
            }
        }
        p->aggs.push_back(m);
    }
    if (accs.size() > 16) return fail(unsupported("more than 16 distinct accumulators"));
    for (auto &aq : accs) {
        ph::JitShape::Acc A;
        A.op = aq.op;
        long double b = 1;
        for (auto &f : aq.pr.f) {
            const auto &c = t->cols[(size_t)f.col];
            if (!c.has_range) return fail(unsupported("a summed column has no range statistics"));
            int sl = slot_of(f.col);
            if (sl < 0) return fail(unsupported("aggregate column type"));
            bool pure = f.A == 0 && f.B == 1;
            A.factors.push_back({sl, pure});
            if (!pure) { consts.push_back(f.A); consts.push_back(f.B); }
            b *= ph::affine_bound(f, c.min, c.max);
        }
        if (aq.op == 0) row_bound = std::max(row_bound, b);
        S.accs.push_back(A);
    }
    if (tcol.empty()) return fail(unsupported("the plan reads no column"));   // count(*) without predicates
    if ((int)tcol.size() > ph::JIT_MAX_COLS || (int)consts.size() > ph::JIT_MAX_CONSTS) return fail(unsupported("too many columns / constants"));
    const int na = (int)S.accs.size();
    S.lds_cols = ph::JitShape::fit_lds_cols(S.nslots, na);
    if (S.lds_cols == 0) return fail(unsupported("group slots x accumulators exceed the CU's LDS"));
    // Bytes in flight: a workgroup keeps one 1024-row tile prefetched, i.e. 1024 x (row bytes). The
    // 34 B/row of Q1 (34 KiB per CU) covers the HBM latency-bandwidth product with one workgroup
    // per CU; narrower plans need proportionally more resident workgroups (measured: 9 B/row at one
    // workgroup per CU reads 4.0 TB/s, latency bound), as far as their LDS accumulators allow.
    int row_bytes = 0;
    for (int w : S.col_width) row_bytes += w;
    int per_cu = std::max(1, std::min(8, (34 + row_bytes - 1) / row_bytes));
    const int64_t lds_bytes = (int64_t)S.nslots * (na * 8 + 8) * S.lds_cols;
    while (per_cu > 1 && per_cu * lds_bytes > 150 * 1024) per_cu--;
    p->row_bound = row_bound;
    p->bytes_per_row = row_bytes;
    p->jshape = S;
    for (size_t i = 0; i < tcol.size(); i++) p->jparams.col[i] = t->cols[(size_t)tcol[i]].data;
    for (size_t i = 0; i < consts.size(); i++) p->jparams.k[i] = consts[i];
    p->nslots = S.nslots; p->stride = na + 2; p->cnt_idx = na; p->first_idx = na + 1;
    for (auto &A : S.accs) p->ops.push_back(A.op);
    p->ops.push_back(0);
    p->ops.push_back(1);
    p->nacc = p->nslots * p->stride;
    p->max_grid = ctx->cu_count * per_cu;
    int rc = ph::jit_get(ctx, S, &p->jkernel);
    if (rc != PH_OK) return fail(rc == PH_EHIP ? PH_EUNSUPPORTED : rc);   // no hiprtc / compile trouble: the generic chain still runs
    rc = plan_alloc(p);
    if (rc != PH_OK) return fail(rc);
    *out = p;
    return PH_OK;
}

// ---------------------------------------------------------------- generic plans
// Any Agg <- Scan(filter) descriptor outside the fused shapes still runs on the device, as the
// chain the operator-granular executors would run: ph_filter_select per conjunct (narrowing the
// selection) -> ph_expr_eval per aggregate argument -> ph_agg_sink -> ph_agg_finalize.

extern "C" int ph_scan_plan_create(ph_ctx *ctx, const ph_table *t, const ph_pred *preds,
                                   int32_t npreds, const int32_t *group_cols, int32_t ngroup_cols,
                                   const ph_aggexpr *aggs, int32_t naggs, ph_scan_plan **out) {
    PH_REQUIRE(ctx && t && out && naggs > 0 && aggs && npreds >= 0 && ngroup_cols >= 0,
               "ph_scan_plan_create: bad arguments");
    const int jit_mode = jit_switch();
    const std::vector<ColView> views = col_views(t);
    int rc = PH_EUNSUPPORTED;
    if (jit_mode == 1) rc = try_jit(ctx, t, views, preds, npreds, group_cols, ngroup_cols, aggs, naggs, out);
    if (rc == PH_EUNSUPPORTED) rc = try_fused(ctx, t, views, preds, npreds, group_cols, ngroup_cols, aggs, naggs, jit_mode == 0, out);
    if (rc == PH_EUNSUPPORTED && jit_mode != 0 && jit_mode != 1) rc = try_jit(ctx, t, views, preds, npreds, group_cols, ngroup_cols, aggs, naggs, out);
    if (rc != PH_EUNSUPPORTED) return rc;
    PH_REQUIRE(ngroup_cols <= 4 && naggs <= 16, "ph_scan_plan_create: at most 4 group columns and 16 aggregates");
    ph_scan_plan *p = new ph_scan_plan();
    p->ctx = ctx;
    p->t = t;
    p->kind = PK_GENERIC;
    p->g_pred_strs.resize((size_t)npreds);
    for (int32_t i = 0; i < npreds; i++) {
        p->g_preds.push_back(preds[i]);
        if (preds[i].k.s) p->g_pred_strs[(size_t)i] = preds[i].k.s;
        if (preds[i].col < 0 || preds[i].col >= (int32_t)t->cols.size()) { delete p; set_error("predicate column %d out of range", preds[i].col); return PH_EINVAL; }
    }
    for (int32_t i = 0; i < ngroup_cols; i++) {
        if (group_cols[i] < 0 || group_cols[i] >= (int32_t)t->cols.size()) { delete p; set_error("group column %d out of range", group_cols[i]); return PH_EINVAL; }
        p->g_groups.push_back(group_cols[i]);
    }
    p->nkeys = ngroup_cols;
    std::vector<ph_col> protos(t->cols.size());
    for (size_t c = 0; c < t->cols.size(); c++) { protos[c].type = t->cols[c].type; protos[c].scale = t->cols[c].scale; }
    for (int32_t a = 0; a < naggs; a++) {
        p->g_aggs.push_back(aggs[a]);
        ph_scan_plan::AggMap m{aggs[a].kind, a, 0};
        if (aggs[a].kind != PH_A_COUNT_STAR) {
            int rc2 = ph_expr_scale(protos.data(), aggs[a].prog, aggs[a].nprog, &m.scale);
            if (rc2 != PH_OK) { delete p; return rc2; }
        }
        p->aggs.push_back(m);
    }
    *out = p;
    return PH_OK;
}

static int generic_run(ph_scan_plan *p, int64_t row_begin, int64_t row_end) {
    ph_ctx *ctx = p->ctx;
    const ph_table *t = p->t;
    int64_t n = row_end - row_begin;
    // device views of the table columns, shifted to row_begin
    std::vector<ph_col> cols(t->cols.size());
    for (size_t c = 0; c < t->cols.size(); c++) {
        const auto &d = t->cols[c];
        ph_col v{};
        v.type = d.type; v.scale = d.scale; v.aux = d.aux; v.aux_bytes = d.aux_bytes;
        int w = d.type == PH_STR ? 4 : ph::type_width(d.type);
        v.data = (const char *)d.data + row_begin * w;
        if (d.validity) {
            PH_REQUIRE(row_begin % 8 == 0, "generic plan over NULL-able columns needs row_begin %% 8 == 0");
            v.validity = d.validity + row_begin / 8;
        }
        cols[c] = v;
    }
    if (p->g_agg) { ph_agg_free(p->g_agg); p->g_agg = nullptr; }
    std::vector<int32_t> key_types;
    for (int32_t g : p->g_groups) key_types.push_back(t->cols[(size_t)g].type);
    if (key_types.empty()) key_types.push_back(PH_I32);
    std::vector<ph_aggspec> specs;
    for (size_t a = 0; a < p->g_aggs.size(); a++) specs.push_back(ph_aggspec{p->g_aggs[a].kind, (int32_t)a});
    PH_CHECK(ph_agg_create(ctx, (int32_t)key_types.size(), key_types.data(), (int32_t)specs.size(), specs.data(), 1024, &p->g_agg));
    if (n <= 0) return PH_OK;
    std::vector<void *> temps;
    auto cleanup = [&]() { for (void *q : temps) ctx->pool_release(q); };
    auto fail = [&](int rc) { cleanup(); return rc; };
    // ---- conjuncts narrow the selection one after the other (execSelectAnd)
    int32_t *sel = nullptr;
    int64_t cnt = n;
    for (size_t i = 0; i < p->g_preds.size() && cnt > 0; i++) {
        ph_pred pr = p->g_preds[i];
        pr.k.s = p->g_pred_strs[i].empty() ? nullptr : p->g_pred_strs[i].c_str();
        const auto &d = t->cols[(size_t)pr.col];
        if (d.type == PH_CODE8 && pr.k.type == PH_STR) {  // literal -> dictionary code
            int code = 999;
            for (size_t k = 0; k < d.dict.size(); k++) if (pr.k.s && d.dict[k] == pr.k.s) code = (int)k;
            pr.k.type = PH_I32;
            pr.k.i = code;
        }
        int32_t *out = nullptr;
        if (ctx->pool_alloc(cnt * 4, (void **)&out) != PH_OK) return fail(PH_EHIP);
        temps.push_back(out);
        int64_t m = 0;
        int rc = ph_filter_select(ctx, &cols[(size_t)pr.col], n, pr.op, &pr.k, sel, cnt, out, &m);
        if (rc != PH_OK) return fail(rc);
        sel = out;
        cnt = m;
    }
    if (cnt == 0) { cleanup(); return PH_OK; }
    // ---- keys
    std::vector<ph_col> keys;
    for (int32_t g : p->g_groups) keys.push_back(cols[(size_t)g]);
    if (keys.empty()) {
        void *zero = nullptr;
        int64_t span = sel ? n : cnt;  // addressed by row id
        if (ctx->pool_alloc(span * 4, &zero) != PH_OK) return fail(PH_EHIP);
        temps.push_back(zero);
        if (hipMemsetAsync(zero, 0, (size_t)span * 4, ctx->stream) != hipSuccess) return fail(PH_EHIP);
        ph_col c{}; c.type = PH_I32; c.data = zero;
        keys.push_back(c);
    }
    // ---- aggregate arguments, evaluated positionally over the selected rows
    bool any_validity = false;
    for (auto &c : cols) any_validity |= c.validity != nullptr;
    std::vector<ph_col> args(p->g_aggs.size());
    for (size_t a = 0; a < p->g_aggs.size(); a++) {
        const ph_aggexpr &ax = p->g_aggs[a];
        if (ax.kind == PH_A_COUNT_STAR) continue;
        void *out = nullptr, *val = nullptr;
        if (ctx->pool_alloc(cnt * 8, &out) != PH_OK) return fail(PH_EHIP);
        temps.push_back(out);
        if (any_validity) { if (ctx->pool_alloc((cnt + 7) / 8 + 64, &val) != PH_OK) return fail(PH_EHIP); temps.push_back(val); }
        int rc = ph_expr_eval(ctx, cols.data(), (int32_t)cols.size(), ax.prog, ax.nprog, sel, cnt, (int64_t *)out, (uint8_t *)val);
        if (rc != PH_OK) return fail(rc);
        ph_col c{}; c.type = PH_DEC64; c.scale = p->aggs[a].scale; c.data = out; c.validity = (const uint8_t *)val;
        args[a] = c;
    }
    int rc = ph_agg_sink(p->g_agg, keys.data(), args.data(), (int32_t)args.size(), sel, cnt, 1, 0);
    if (rc == PH_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = PH_EHIP;
    cleanup();
    return rc;
}

static int generic_fetch(ph_scan_plan *p, ph_agg_result **out) {
    int64_t ng = 0;
    PH_CHECK(ph_agg_group_count(p->g_agg, &ng));
    int naggs = (int)p->aggs.size();
    size_t g = (size_t)std::max<int64_t>(ng, 1), nk = (size_t)std::max<int>(p->nkeys, 1);
    ph_agg_result *r = (ph_agg_result *)calloc(1, sizeof *r);
    r->ngroups = ng;
    r->nkeys = p->nkeys;
    r->naggs = naggs;
    r->first_row = (int64_t *)calloc(g, 8);
    r->keys = (int64_t *)calloc(g * nk, 8);
    r->sum_lo = (uint64_t *)calloc(g * naggs, 8);
    r->sum_hi = (int64_t *)calloc(g * naggs, 8);
    r->count = (uint64_t *)calloc(g * naggs, 8);
    r->scale = (int32_t *)calloc((size_t)naggs, 4);
    for (int a = 0; a < naggs; a++) r->scale[a] = p->aggs[(size_t)a].scale;
    std::vector<uint8_t> knull(g * nk);
    int rc = ph_agg_finalize(p->g_agg, (int64_t)g, r->first_row, r->keys, knull.data(), r->sum_lo, r->sum_hi, r->count);
    if (rc != PH_OK) { ph_agg_result_free(r); return rc; }
    *out = r;
    return PH_OK;
}

// ---------------------------------------------------------------- a run of a fused plan, step by step

// at every run: PH_SCAN_GRID; for lowcard_chain PH_SCAN_HIST, and PH_SCAN_UNROLL where the wide kernel runs
static ph::ScanSwitches run_switches(const ph_scan_plan *p) {
    ph::ScanSwitches sw = process_switches();
    if (const char *e = getenv("PH_SCAN_GRID")) sw.grid = atoi(e);
    if (p->kind == PK_LOWCARD_CHAIN) {
        sw.hist = hist_switch();
        if (p->lc.form == ph::FORM_WIDE)
            if (const char *e = getenv("PH_SCAN_UNROLL")) sw.unroll = atoi(e);
    }
    return sw;
}

// A lean lowcard_chain plan at the start of a run over `rows` rows: the table's packed scan group of the plan's columns when it exists or
// when this run triggers its build (ph::scan_group_for) becomes the plan's input from this launch on: the group's address and layout are
// kept in p->lc, the variant is "packed64" and the kernel loads 8 bytes a row ("split56" and 7 over a group in the split form). No group:
// nothing changes.
static int bind_scan_group(ph_scan_plan *p, int64_t rows, const ph::ScanSwitches &sw) {
    if (p->lc.pk || !ph::lc_takes_lean(lc_facts(p->lc, true), sw)) return PH_OK;
    ph_table::scangroup g;
    const int rc = ph::scan_group_for(p->ctx, const_cast<ph_table *>(p->t), p->lc_cols, rows, false, &g);
    if (rc == PH_EUNSUPPORTED) return PH_OK;
    PH_CHECK(rc);
    if (g.nk1 != p->lc.nk1 || g.nslots != p->lc.nslots) return PH_OK;   // (both come from the same dictionaries)
    for (int f = 0; f < ph::PACK_NFIELDS; f++) {
        p->lc.pk_shift[f] = (uint8_t)g.shift[f];
        p->lc.pk_width[f] = (uint8_t)g.width[f];
    }
    p->lc.pk = (const uint8_t *)g.data;
    p->lc.pk_form = (int16_t)g.form;
    p->bytes_per_row = g.form == ph::SG_SPLIT56 ? 7 : 8;
    return PH_OK;
}

// One host-visible result per run without a publish launch (PH_SCAN_TAIL=0: merge kernel, then publish_kernel at the fetch). The one-group
// sum kernel (Q6 shape: two words per workgroup) merges AND publishes in its last workgroup — one launch per run; for the others the merge
// kernel's last wave publishes — two launches (a single workgroup folding 42 words x 256 workgroups was slower than the 42-wave merge launch).
// back_to_back: the last run's result was never fetched, so nothing is published (ph_scan_plan::unfetched).
static int arm_tail(ph_scan_plan *p, bool back_to_back, ph::ScanTail *tail) {
    *tail = ph::ScanTail{};
    if (!process_switches().tail || p->nacc > ph::SCAN_TAIL_MAX_ACC || (back_to_back && p->kind != PK_FILTER_SUMPROD)) return PH_OK;
    ph_ctx *ctx = p->ctx;
    if (!ctx->scan_done_dev) {   // the ticket: zero between launches
        PH_HIP(hipMalloc((void **)&ctx->scan_done_dev, 64));
        PH_HIP(hipMemsetAsync(ctx->scan_done_dev, 0, 64, ctx->stream));
    }
    tail->done = ctx->scan_done_dev;
    tail->out_lo = p->out_lo;
    tail->out_hi = p->out_hi;
    tail->nacc = p->nacc;
    if (!back_to_back) PH_CHECK(ctx->arm_publish((int64_t)p->nacc * 16, &tail->mbox, &tail->flag, &tail->seq));
    p->armed_seq = tail->seq;
    return PH_OK;
}

static int launch_filter_sumprod_plan(ph_scan_plan *p, int64_t row_begin, int64_t rows, const ph::ScanSwitches &sw, int grid, const ph::ScanTail &tail) {
    ph::FilterSumProdParams P = p->fs;
    P.row_begin = row_begin;
    P.row_end = row_begin + rows;
    P.partials = p->partials;
    P.tail = tail;
    P.tail.min_stride = 0;
    PH_CHECK(ph::launch_filter_sumprod(p->ctx, P, ph::fs_choose(fs_facts(P), sw), sw, grid));
    if (!tail.done) PH_CHECK(ph::launch_merge_partials(p->ctx, p->partials, grid, 2, 0, p->out_lo, p->out_hi));
    return PH_OK;
}

static int launch_jit_plan(ph_scan_plan *p, int64_t row_begin, int64_t rows, int grid, const ph::ScanTail &tail) {
    ph::JitParams P = p->jparams;
    P.row_begin = row_begin;
    P.row_end = row_begin + rows;
    P.partials = p->partials;
    PH_CHECK(ph::jit_launch(p->ctx, p->jkernel, P, grid));
    unsigned long long opmask = 0;
    for (int j = 0; j < p->stride; j++) opmask |= (unsigned long long)p->ops[(size_t)j] << (2 * j);
    return ph::launch_merge_partials_ops(p->ctx, p->partials, grid, p->nacc, p->stride, opmask, p->out_lo, p->out_hi, &tail);
}

static int launch_lowcard_chain_plan(ph_scan_plan *p, int64_t row_begin, int64_t rows, ph::LcInst inst, const ph::ScanSwitches &sw, int grid,
                                     const ph::ScanTail &tail) {
    ph::LowcardChainParams P = p->lc;
    P.row_begin = row_begin;
    P.row_end = row_begin + rows;
    P.partials = p->partials;
    P.tail = ph::ScanTail{};
    P.bins = ph::lc_takes_bins(inst);
    PH_CHECK(ph::launch_lowcard_chain(p->ctx, P, inst, sw, grid));
    return ph::launch_merge_partials(p->ctx, p->partials, grid, p->nacc, ph::LC_NACC + 1, p->out_lo, p->out_hi, &tail);
}

extern "C" int ph_scan_plan_run(ph_scan_plan *p, int64_t row_begin, int64_t row_end) {
    // ---- validate
    PH_REQUIRE(p != nullptr, "ph_scan_plan_run: plan is NULL");
    // the narrow kernels mask the rows below row_begin, so any row_begin will do; every other kernel loads 4-row vectors from row_begin on
    const bool narrow = (p->kind == PK_FILTER_SUMPROD && p->fs.form != ph::FORM_WIDE) || (p->kind == PK_LOWCARD_CHAIN && p->lc.form != ph::FORM_WIDE);
    PH_REQUIRE(row_begin >= 0 && row_end >= row_begin && row_end <= p->t->nrows && (narrow || row_begin % 4 == 0),
               "ph_scan_plan_run: rows [%lld,%lld) invalid (begin must be a multiple of 4 unless the plan reads narrowed copies; table has %lld rows)",
               (long long)row_begin, (long long)row_end, (long long)p->t->nrows);
    if (p->kind == PK_GENERIC) return generic_run(p, row_begin, row_end);
    const ph::ScanSwitches sw = run_switches(p);
    const bool lowcard = p->kind == PK_LOWCARD_CHAIN;
    // ---- the packed scan group, the geometry, the instance
    if (lowcard) PH_CHECK(bind_scan_group(p, row_end - row_begin, sw));
    const int64_t rows = p->never ? 0 : row_end - row_begin;
    const bool bins_eligible = lowcard && ph::lc_takes_bins(ph::lc_choose(lc_facts(p->lc, true), sw));
    const int64_t anchor = lowcard && p->lc.pk && p->lc.pk_form == ph::SG_SPLIT56 ? 4096 : 16;   // a split group's tiles start at multiples of 4096
    const ph::ScanGeometry g = ph::scan_geometry(row_begin, rows, narrow, p->max_grid, sw.grid, bins_eligible, partials_cap(p), anchor);
    const ph::LcInst inst = lowcard ? ph::lc_choose(lc_facts(p->lc, g.bins), sw) : ph::LCI_WIDE;
    if (lowcard) p->last_inst = inst;
    // ---- overflow proof: a workgroup's int64 partial sums at most rows_per_block values of magnitude <= row_bound
    const long double rows_per_block = (long double)((g.tiles + g.grid - 1) / g.grid) * (long double)g.tile_rows;
    if (p->row_bound * rows_per_block >= 4.0e18L) {
        set_error("decimal overflow proof failed: per-row bound %.3Lg x %.0Lf rows per workgroup", p->row_bound, rows_per_block);
        return PH_EOVERFLOW;
    }
    p->last_rows = rows;
    p->last_grid = g.grid;
    p->armed_seq = 0;
    // ---- the tail, the launches
    const bool back_to_back = p->unfetched;
    p->unfetched = true;
    ph::ScanTail tail;
    PH_CHECK(arm_tail(p, back_to_back, &tail));
    if (p->kind == PK_FILTER_SUMPROD) return launch_filter_sumprod_plan(p, row_begin, rows, sw, g.grid, tail);
    if (p->kind == PK_JIT) return launch_jit_plan(p, row_begin, rows, g.grid, tail);
    return launch_lowcard_chain_plan(p, row_begin, rows, inst, sw, g.grid, tail);
}

extern "C" void ph_agg_result_free(ph_agg_result *r) {
    if (!r) return;
    free(r->first_row); free(r->keys); free(r->sum_lo); free(r->sum_hi); free(r->count); free(r->scale); free(r->key_null);
    free(r);
}

// result rows from raw accumulator words (lo[nacc], hi[nacc]); first-row words are global ids
static int assemble(ph_scan_plan *p, const std::vector<unsigned long long> &lo, const std::vector<long long> &hi,
                    ph_agg_result **out) {
    int naggs = (int)p->aggs.size();
    struct G { int64_t first; int slot; };
    std::vector<G> groups;
    const int stride = p->stride;
    for (int s = 0; s < p->nslots; s++)
        if (lo[(size_t)s * stride + p->cnt_idx] > 0)
            groups.push_back({p->first_idx >= 0 ? (int64_t)lo[(size_t)s * stride + p->first_idx] : 0, s});
    std::sort(groups.begin(), groups.end(), [](const G &a, const G &b) { return a.first < b.first; });
    ph_agg_result *r = (ph_agg_result *)calloc(1, sizeof *r);
    size_t ng = groups.size(), nk = (size_t)p->nkeys;
    r->ngroups = (int64_t)ng;
    r->nkeys = p->nkeys;
    r->naggs = naggs;
    r->first_row = (int64_t *)calloc(ng ? ng : 1, 8);
    r->keys = (int64_t *)calloc((ng ? ng : 1) * (nk ? nk : 1), 8);
    r->sum_lo = (uint64_t *)calloc((ng ? ng : 1) * naggs, 8);
    r->sum_hi = (int64_t *)calloc((ng ? ng : 1) * naggs, 8);
    r->count = (uint64_t *)calloc((ng ? ng : 1) * naggs, 8);
    r->scale = (int32_t *)calloc((size_t)naggs, 4);
    for (int a = 0; a < naggs; a++) r->scale[a] = p->aggs[(size_t)a].scale;
    for (size_t g = 0; g < ng; g++) {
        int s = groups[g].slot;
        r->first_row[g] = groups[g].first;
        int rem = s;   // slot = dense index over the group columns' dictionaries, last column fastest
        for (int c = (int)nk - 1; c >= 0; c--) {
            r->keys[g * nk + (size_t)c] = rem % p->gcard[(size_t)c];
            rem /= p->gcard[(size_t)c];
        }
        uint64_t cnt = lo[(size_t)s * stride + p->cnt_idx];
        for (int a = 0; a < naggs; a++) {
            const auto &m = p->aggs[(size_t)a];
            r->count[g * naggs + a] = cnt;  // no NULL inputs on this path
            if (m.kind == PH_A_COUNT_STAR || m.kind == PH_A_COUNT) continue;
            size_t idx = (size_t)s * stride + (size_t)m.acc;
            r->sum_lo[g * naggs + a] = lo[idx];
            r->sum_hi[g * naggs + a] = hi[idx];
        }
    }
    *out = r;
    return PH_OK;
}

extern "C" int ph_scan_plan_fetch(ph_scan_plan *p, ph_agg_result **out) {
    PH_REQUIRE(p && out, "ph_scan_plan_fetch: bad arguments");
    if (p->kind == PK_GENERIC) {
        PH_REQUIRE(p->g_agg != nullptr, "ph_scan_plan_fetch: run the plan first");
        return generic_fetch(p, out);
    }
    // lo[nacc] and hi[nacc] are ONE allocation (plan_alloc): one host round trip for both (two cost ~45 us more per query)
    std::vector<unsigned long long> words((size_t)p->nacc * 2);
    const int armed = p->ctx->collect_armed(words.data(), (int64_t)words.size() * 8, p->armed_seq);   // 1: the mailbox has been used since
    p->armed_seq = 0;
    p->unfetched = false;
    if (armed < 0) return armed;
    if (armed == 1) PH_CHECK(p->ctx->download(words.data(), p->out_lo, (int64_t)words.size() * 8));
    std::vector<unsigned long long> lo(words.begin(), words.begin() + p->nacc);
    std::vector<long long> hi((size_t)p->nacc);
    memcpy(hi.data(), words.data() + p->nacc, (size_t)p->nacc * 8);
    return assemble(p, lo, hi, out);
}

extern "C" int ph_scan_plan_partials_dev(ph_scan_plan *p, void **dev, int32_t *nwords) {
    PH_REQUIRE(p && dev && nwords, "ph_scan_plan_partials_dev: bad arguments");
    if (p->kind == PK_GENERIC) { set_error("generic plans keep their state in a hash table, not in a fixed partial array"); return PH_EUNSUPPORTED; }
    *dev = p->out_lo;
    *nwords = 2 * p->nacc;
    return PH_OK;
}

extern "C" int ph_scan_plan_fetch_merged(ph_scan_plan *p, const uint64_t *words, int32_t nranks, ph_agg_result **out) {
    PH_REQUIRE(p && words && out && nranks >= 1, "ph_scan_plan_fetch_merged: bad arguments");
    if (p->kind == PK_GENERIC) { set_error("ph_scan_plan_fetch_merged: fused plans only"); return PH_EUNSUPPORTED; }
    size_t n = (size_t)p->nacc;
    std::vector<unsigned long long> lo(n, 0);
    std::vector<long long> hi(n, 0);
    for (size_t j = 0; j < n; j++) {
        const int wi = (int)(j % (size_t)p->stride);
        const int op = p->ops[(size_t)wi];
        if (wi == p->first_idx) {
            lo[j] = ~0ull;
            for (int32_t r = 0; r < nranks; r++) {
                const uint64_t *w = words + (size_t)r * 2 * n;
                // first-seen row across ranks: rank r's rows come after rank r-1's
                if (w[j] != 0xffffffffull && w[j] != (uint64_t)INT64_MAX) {
                    unsigned long long gfirst = ((unsigned long long)r << 40) + w[j];
                    if (gfirst < lo[j]) lo[j] = gfirst;
                }
            }
        } else if (op == 0) {
            for (int32_t r = 0; r < nranks; r++) {
                const uint64_t *w = words + (size_t)r * 2 * n;
                unsigned long long nl = lo[j] + w[j];
                hi[j] += (long long)w[n + j] + (nl < lo[j] ? 1 : 0);
                lo[j] = nl;
            }
        } else {   // MIN / MAX words are plain int64 values (identity when a rank saw no row)
            long long best = op == 1 ? INT64_MAX : INT64_MIN;
            for (int32_t r = 0; r < nranks; r++) {
                long long v = (long long)words[(size_t)r * 2 * n + j];
                best = op == 1 ? std::min(best, v) : std::max(best, v);
            }
            lo[j] = (unsigned long long)best;
            hi[j] = best < 0 ? -1 : 0;
        }
    }
    return assemble(p, lo, hi, out);
}

extern "C" int ph_scan_filter_agg(ph_ctx *ctx, const ph_table *t, int64_t row_begin, int64_t row_end,
                                  const ph_pred *preds, int32_t npreds, const int32_t *group_cols,
                                  int32_t ngroup_cols, const ph_aggexpr *aggs, int32_t naggs,
                                  ph_agg_result **out) {
    ph_scan_plan *p = nullptr;
    PH_CHECK(ph_scan_plan_create(ctx, t, preds, npreds, group_cols, ngroup_cols, aggs, naggs, &p));
    int rc = ph_scan_plan_run(p, row_begin, row_end);
    if (rc == PH_OK) rc = ph_scan_plan_fetch(p, out);
    ph_scan_plan_free(p);
    return rc;
}
