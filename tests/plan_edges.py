"""Constructed tables, plain references and the case list of the ph_plan edge tests (test_gpu_plan_edges.py; checked on their own, without a
device, by test_plan_edges_reference.py).

ph_plan picks, per join, one of about fifteen forms (JoinWork::* and lower_node in plan_exec.hip) from table statistics and relation
properties. TPC-H data never shows those forms a filter that empties a side, a probe side where every row misses, a declared-unique key that
is not, one-row tables, fan-out past a 16-row run or keys at the ends of the integer domains. Every case here is ONE description — tables as
numpy columns and a plan as nested dicts — read twice: test_gpu_plan_edges.py lowers it into a hip.Plan, ref_plan() below evaluates it with
ref_filter / ref_join / ref_agg. The two cannot drift apart, and the reference shares nothing with the library or with oracle/: joins are
sort + searchsorted over the key VALUES, aggregates are Python ints in a dict. Integers are exact, so nothing here has a tolerance.

Nothing in this file touches a device or calls the library."""
import functools

import numpy as np

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1

# ------------------------------------------------------------------ reference operators
OPS = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}


def ref_filter(values, op, k, valid=None):
    """rows where `values OP k` holds: k a constant or a column of the same rows (column-vs-column); a NULL never qualifies. A bool mask."""
    m = OPS[op](np.asarray(values), k)
    return m if valid is None else m & valid


def _key_ids(probe_keys, build_keys):
    """the key tuples of both sides as int64 ids that are equal exactly where the tuples are (one int column: its values)"""
    if not isinstance(probe_keys, (list, tuple)):
        probe_keys, build_keys = [probe_keys], [build_keys]
    pid = bid = None
    for pk, bk in zip(probe_keys, build_keys):
        pk, bk = np.asarray(pk), np.asarray(bk)
        if len(probe_keys) == 1 and pk.dtype != object:
            return pk.astype(np.int64), bk.astype(np.int64)
        _, inv = np.unique(np.concatenate([pk, bk]), return_inverse=True)
        a, b = inv[:len(pk)].astype(np.int64), inv[len(pk):].astype(np.int64)
        width = int(inv.max()) + 1 if len(inv) else 1
        pid, bid = (a, b) if pid is None else (pid * width + a, bid * width + b)
    return pid, bid


def ref_join(kind, probe_keys, build_keys, residual=None):
    """SQL equi-join on one key column per side or a list of them. residual(probe_row, build_row) -> bool mask over the pairs.
    inner: (probe_row, build_row) of every pair (that passes the residual); left: those, then every probe row without one, with build row -1;
    semi / anti: the probe rows with / without a pair, ascending."""
    pid, bid = _key_ids(probe_keys, build_keys)
    order = np.argsort(bid, kind="stable")
    sb = bid[order]
    lo, hi = np.searchsorted(sb, pid, "left"), np.searchsorted(sb, pid, "right")
    cnt = hi - lo
    pr = np.repeat(np.arange(len(pid), dtype=np.int64), cnt)
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    br = order[np.repeat(lo, cnt) + within].astype(np.int64)
    if residual is not None:
        keep = np.asarray(residual(pr, br), dtype=bool)
        pr, br = pr[keep], br[keep]
    if kind == "inner":
        return pr, br
    has = np.zeros(len(pid), dtype=bool)
    has[pr] = True
    if kind == "semi":
        return np.nonzero(has)[0]
    if kind == "anti":
        return np.nonzero(~has)[0]
    assert kind == "left"                               # (a residual is part of ON: a probe row whose pairs all fail it has no pair)
    un = np.nonzero(~has)[0]
    return np.concatenate([pr, un]), np.concatenate([br, np.full(len(un), -1, dtype=np.int64)])


def ref_agg(group_cols, aggs, n):
    """GROUP BY over n rows. group_cols: [(values, valid or None)]; aggs: [(kind, values, valid or None)], kind one of count_star, count, sum,
    min, max, avg, count_distinct. A group column holds integers or bytes (VARCHAR). {key tuple (None = NULL): [result per aggregate]}: counts
    are ints (count_distinct: the number of different non-NULL inputs), sum / min / max Python ints or None (NULL: no non-NULL input), avg the
    pair (sum, count) or None. No group column = one global group, present also over zero rows."""
    if n > 500_000:
        return _ref_agg_big(group_cols, aggs, n)
    gl = [[None if (v is not None and not v[i]) else (c[i] if isinstance(c[i], bytes) else int(c[i])) for i in range(n)] for c, v in group_cols]
    al = [(kind, None if vals is None else [int(x) for x in vals], None if valid is None else [bool(x) for x in valid]) for kind, vals, valid in aggs]
    state = {}
    if not group_cols:
        state[()] = [[0, 0, None, None, set()] for _ in aggs]
    for i in range(n):
        st = state.setdefault(tuple(g[i] for g in gl), None)
        if st is None:
            st = state[tuple(g[i] for g in gl)] = [[0, 0, None, None, set()] for _ in aggs]
        for a, (kind, vals, valid) in enumerate(al):
            s = st[a]                                   # rows, non-NULL inputs, sum, (min, max), the different inputs
            s[0] += 1
            if kind == "count_star" or (valid is not None and not valid[i]):
                continue
            x = vals[i]
            s[1] += 1
            s[2] = x if s[2] is None else s[2] + x
            s[3] = (x, x) if s[3] is None else (min(s[3][0], x), max(s[3][1], x))
            s[4].add(x)
    out = {}
    for key, st in state.items():
        row = []
        for (kind, _, _), s in zip(al, st):
            if kind == "count_star":
                row.append(s[0])
            elif kind == "count":
                row.append(s[1])
            elif kind == "count_distinct":
                row.append(len(s[4]))
            elif s[1] == 0:
                row.append(None)
            else:
                row.append({"sum": s[2], "min": s[3][0], "max": s[3][1], "avg": (s[2], s[1])}[kind])
        out[key] = row
    return out


def _ref_agg_big(group_cols, aggs, n):
    """ref_agg for the clustered table's millions of rows, where a Python loop per row takes a minute: ONE NULL-free integer group column, NULL-free
    arguments whose absolute values sum below 2^62 — so int64 sums cannot wrap and are the exact integers. Pinned against the loop by
    test_plan_edges_reference.py."""
    assert len(group_cols) == 1 and group_cols[0][1] is None and all(valid is None for _, _, valid in aggs)
    keys, inv = np.unique(np.asarray(group_cols[0][0], dtype=np.int64), return_inverse=True)
    rows = np.bincount(inv, minlength=len(keys))
    per = []
    for kind, vals, _ in aggs:
        if kind in ("count_star", "count"):
            per.append(rows.tolist())
            continue
        x = np.asarray(vals, dtype=np.int64)
        assert int(np.abs(x).astype(np.float64).sum()) < 2 ** 62
        if kind in ("sum", "avg"):
            s = np.zeros(len(keys), dtype=np.int64)
            np.add.at(s, inv, x)
            per.append([(int(v), int(c)) for v, c in zip(s, rows)] if kind == "avg" else s.tolist())
        else:
            m = np.full(len(keys), I64_MAX if kind == "min" else I64_MIN, dtype=np.int64)
            (np.minimum if kind == "min" else np.maximum).at(m, inv, x)
            per.append(m.tolist())
    return {(int(k),): [p[g] for p in per] for g, k in enumerate(keys)}


# ------------------------------------------------------------------ tables: numpy columns + what the catalog declares
def C(typ, arr, scale=0, dictionary=None):
    """one column: typ in i32, date (int32 days), i64, dec (int64 unscaled + scale), code (uint8 + dictionary), str (an object array of bytes)"""
    dt = {"i32": np.int32, "date": np.int32, "i64": np.int64, "dec": np.int64, "code": np.uint8, "str": object}[typ]
    return dict(typ=typ, arr=np.asarray(arr, dtype=dt), scale=scale, dictionary=dictionary)


def T(cols, unique=()):
    return dict(cols=cols, n=len(cols[0]["arr"]), unique=[list(u) for u in unique])


# key-domain placements: (key type, first key of a range of n keys, distance between two keys)
def placement(place, n):
    if place == "i32_min":
        return "i32", I32_MIN, 1            # an int32 range that starts at INT32_MIN
    if place == "i32_max":
        return "i32", I32_MAX - (n - 1), 1  # an int32 range that ends at INT32_MAX
    if place == "i32_mid":
        return "i32", 1000, 1
    if place == "i64_sparse":
        return "i64", -(n // 2) << 33, 1 << 33   # k << 33: no dense range, so no direct table
    if place == "i64_max":
        return "i64", I64_MAX - (n - 1), 1  # an int64 range that ends at INT64_MAX
    raise KeyError(place)


def _keys(typ, vals):
    lo, hi = (I32_MIN, I32_MAX) if typ == "i32" else (I64_MIN, I64_MAX)
    assert all(lo <= v <= hi for v in (min(vals), max(vals))) if len(vals) else True
    return np.array(vals, dtype=np.int32 if typ == "i32" else np.int64)


DIM_KEY, DIM_PAY, DIM_ATTR, DIM_CODE, ND = 0, 1, 2, 3, 4
ATTR_DICT = ["A0", "A1", "A2", "A3", "A4"]


def dim(n, place="i32_mid", shuffle=False):
    """key (strictly ascending and unique: first + i * step; stored in another order with shuffle), pay DECIMAL(.., 2), attr INTEGER 0..4, the
    same attribute as a dictionary code. The key is declared unique."""
    typ, first, step = placement(place, n)
    i = np.arange(n, dtype=np.int64)
    if shuffle:
        i = (i * 1237 + 11) % n if n > 1 else i      # 1237 is prime and no divisor of the sizes used: a permutation
        assert len(np.unique(i)) == n
    key = _keys(typ, [first + int(x) * step for x in i])
    pay = (i * 2654435761) % 2_000_001 - 1_000_000
    attr = (i * 7 + 3) % 5
    t = T([C(typ, key), C("dec", pay, 2), C("i32", attr), C("code", attr, dictionary=ATTR_DICT)], unique=[[DIM_KEY]])
    t.update(typ=typ, first=first, step=step)
    return t


def dupdim(nkeys, place="i32_mid", fan=(1, 2, 17)):
    """a build side whose key repeats: key number k occurs fan[k % len(fan)] times (17 > the 16-row run the table-less join walks), stored in
    key order; pay DECIMAL(.., 2), attr INTEGER 0..4, z INTEGER 0..99 for column-vs-column conditions. Nothing is declared."""
    typ, first, step = placement(place, nkeys)
    reps = np.array([fan[k % len(fan)] for k in range(nkeys)], dtype=np.int64)
    k = np.repeat(np.arange(nkeys, dtype=np.int64), reps)
    i = np.arange(len(k), dtype=np.int64)
    t = T([C(typ, _keys(typ, [first + int(x) * step for x in k])), C("dec", (i * 40503) % 20_001 - 10_000, 2), C("i32", (i * 7 + 3) % 5), C("i32", (i * 29) % 100)])
    t.update(typ=typ, first=first, step=step, nkeys=nkeys)
    return t


F_KEY, F_AMT, F_X, F_Y, F_ID, NF = 0, 1, 2, 3, 4, 5


def fact(n, d, order="shuffled", dangling="none", dup=3):
    """a foreign key into d (a dim or dupdim): fk, amt DECIMAL(.., 2), x and y INTEGER 0..99 (x < y for column-vs-column conditions), id = the
    row number. order: "shuffled"; "ascending" (clustered: every key `dup` times in a row); "strict" (strictly ascending, n <= d's keys).
    dangling: "none"; "some" (every fifth key is replaced by one d does not have); "all". A dangling key lies below d's range, above it or —
    where d's keys have gaps — between two of them, as far as the key type has room."""
    nk = d.get("nkeys", d["n"])
    typ, first, step = d["typ"], d["first"], d["step"]
    i = np.arange(n, dtype=np.int64)
    if order == "shuffled":
        idx = (i * 2654435761 + 12345) % nk
    elif order == "ascending":
        idx = ((i // dup) * nk) // max(-(-n // dup), 1)
    else:
        assert order == "strict" and n <= nk
        idx = (i * nk) // n
    vals = [first + int(x) * step for x in idx]
    lo, hi = (I32_MIN, I32_MAX) if typ == "i32" else (I64_MIN, I64_MAX)
    last = first + (nk - 1) * step
    outside = []                                       # keys d does not have, one family per position
    if first - 1 >= lo:
        outside.append(lambda j: max(first - 1 - j, lo))
    if last + 1 <= hi:
        outside.append(lambda j: min(last + 1 + j, hi))
    if step > 1:
        outside.append(lambda j: first + (j % max(nk - 1, 1)) * step + 1)
    if dangling != "none":
        assert outside
        for r in range(n):
            if dangling == "all" or r % 5 == 2:
                vals[r] = outside[r % len(outside)](r // len(outside))
        if order != "shuffled":
            vals.sort()
            if order == "strict":
                vals = sorted(set(vals))
    m = len(vals)
    i = np.arange(m, dtype=np.int64)
    t = T([C(typ, _keys(typ, vals)), C("dec", (i * 48271) % 200_001 - 100_000, 2), C("i32", (i * 37) % 100), C("i32", (i * 53) % 100), C("i32", i)])
    t.update(typ=typ)
    return t


R_K1, R_K2, R_PAY, NR = 0, 1, 2, 3


def runs(n1, run_len, first=500):
    """a two-column unique key (k1, k2) stored in runs of run_len by k1 (ph_table_col_run_len > 1): row i holds k1 = first + i // run_len and a k2
    that is unique inside the run; pay DECIMAL(.., 2). (k1, k2) is declared unique."""
    assert run_len in (3, 4)
    i = np.arange(n1 * run_len, dtype=np.int64)
    k1, j = first + i // run_len, i % run_len
    k2 = ((i // run_len) * 7 + j * 3) % 1009
    assert all(len(set(k2[r * run_len:(r + 1) * run_len].tolist())) == run_len for r in range(0, n1, max(n1 // 50, 1)))
    t = T([C("i32", k1), C("i32", k2), C("dec", (i * 69621) % 30_001 - 15_000, 2)], unique=[[R_K1, R_K2]])
    t.update(first=first, run_len=run_len, n1=n1)
    return t


F2_K1, F2_K2, F2_AMT, F2_X, F2_ID, NF2 = 0, 1, 2, 3, 4, 5


def fact2(n, r, dangling="none"):
    """a two-column foreign key into runs(): k1, k2, amt, x, id. A dangling row has a k2 no run holds (2000), or a k1 one below or above r's"""
    i = np.arange(n, dtype=np.int64)
    idx = (i * 2654435761 + 777) % r["n"]
    k1, k2 = r["cols"][R_K1]["arr"][idx].astype(np.int64), r["cols"][R_K2]["arr"][idx].astype(np.int64)
    if dangling != "none":
        d = np.ones(n, dtype=bool) if dangling == "all" else (i % 5 == 2)
        which = i % 3
        k2 = np.where(d & (which == 0), 2000, k2)
        k1 = np.where(d & (which == 1), r["first"] - 1, k1)
        k1 = np.where(d & (which == 2), r["first"] + r["n1"], k1)
    return T([C("i32", k1), C("i32", k2), C("dec", (i * 16807) % 50_001 - 25_000, 2), C("i32", (i * 37) % 100), C("i32", i)])


def tiny(keys=(0, 1, 2, 3, 4)):
    """a handful of rows keyed by dim's attr values: key INTEGER (strictly ascending), weight DECIMAL(.., 2)"""
    k = np.array(keys, dtype=np.int64)
    return T([C("i32", k), C("dec", k * 1000 + 7, 2)], unique=[[0]])


BIG_ROWS = (1 << 22) + 3
BIG_RUNS = (1, 2, 16, 17, 40)
BIG_KEY, BIG_A, BIG_B, BIG_ID, NBIG = 0, 1, 2, 3, 4


@functools.lru_cache(maxsize=None)
def clustered():
    """the smallest table clustered_by() accepts (at least 2^22 rows), int32 columns only: key ascending from 0 with run lengths cycling through
    1, 2, 16, 17 and 40 (the table-less join walks 16 rows of a run before it searches for its end), a and b INTEGER 0..99, id = the row number"""
    nk = BIG_ROWS // sum(BIG_RUNS) * len(BIG_RUNS) + len(BIG_RUNS)
    lens = np.tile(np.array(BIG_RUNS, dtype=np.int64), nk // len(BIG_RUNS) + 1)[:nk]
    key = np.repeat(np.arange(nk, dtype=np.int64), lens)[:BIG_ROWS]
    assert len(key) == BIG_ROWS
    i = np.arange(BIG_ROWS, dtype=np.int64)
    t = T([C("i32", key), C("i32", (i * 37) % 100), C("i32", (i * 53) % 100), C("i32", i)])
    t.update(typ="i32", first=0, step=1, nkeys=int(key[-1]) + 1)
    return t


def strings(vals):
    """bytes values as an object array (numpy would make a fixed-width array of them and strip trailing NULs)"""
    out = np.empty(len(vals), dtype=object)
    out[:] = list(vals)
    return out


# ------------------------------------------------------------------ plans as data
def scan(table, preds=(), colcmp=None):
    """all columns of `table` (a name); preds: (table column, op, constant) AND-ed; colcmp: one more conjunct (column, op, column)"""
    return dict(op="scan", table=table, preds=list(preds), colcmp=colcmp)


def join(probe, build, pkeys, bkeys, out, kind="inner", residual=None):
    """out indexes [probe columns | build columns]; residual: (column, op, column) over the same"""
    return dict(op="join", probe=probe, build=build, pkeys=list(pkeys), bkeys=list(bkeys), out=list(out), kind=kind, residual=residual)


def agg(child, groups, aggs):
    """aggs: (kind, child column or None)"""
    return dict(op="agg", child=child, groups=list(groups), aggs=list(aggs))


class Rel:
    """a reference relation: columns as int64 (or object, VARCHAR) arrays, their validity (None = no NULLs), (typ, scale) per column; rid = per
    row, the row of the plan's leftmost table it stems from (None above an aggregate)"""

    def __init__(self, cols, valid, kinds, rid):
        self.cols, self.valid, self.kinds, self.rid = cols, valid, kinds, rid
        self.n = len(cols[0]) if cols else 0

    def take(self, rows, null=None):
        cols, valid = [], []
        for c, v in zip(self.cols, self.valid):
            if null is None:
                cols.append(c[rows])
                valid.append(None if v is None else v[rows])
            else:                                       # rows holds -1 where the side is NULL
                safe = np.where(null, 0, rows)
                cols.append(c[safe] if len(c) else np.zeros(len(rows), dtype=c.dtype))
                valid.append(~null if v is None else (v[safe] & ~null))
        return cols, valid


def _groups_of(node, R):
    return ref_agg([(R.cols[g], R.valid[g]) for g in node["groups"]],
                   [(k, None if c is None else R.cols[c], None if c is None else R.valid[c]) for k, c in node["aggs"]], R.n)


def _eval(node, tables, trace):
    """one node as a relation. trace collects, per scan, join and aggregate in evaluation order, what a test must know about it."""
    if node["op"] == "scan":
        t = tables[node["table"]]
        cols = [c["arr"] if c["typ"] == "str" else c["arr"].astype(np.int64) for c in t["cols"]]
        keep = np.ones(t["n"], dtype=bool)
        for c, op, k in node["preds"]:
            keep &= ref_filter(cols[c], op, k)
        if node["colcmp"]:
            a, op, b = node["colcmp"]
            keep &= ref_filter(cols[a], op, cols[b])
        rows = np.nonzero(keep)[0]
        trace.append(dict(op="scan", table=node["table"], rows=t["n"], kept=len(rows)))
        return Rel([c[rows] for c in cols], [None] * len(cols), [(c["typ"], c["scale"]) for c in t["cols"]], rows)
    if node["op"] == "agg":
        # an aggregate below other operators: its groups as a relation — the key columns, then one column per aggregate, NULL where the
        # aggregate is (counts and sums travel as DECIMALs, sums at their argument's scale)
        R = _eval(node["child"], tables, trace)
        groups = _groups_of(node, R)
        trace.append(dict(op="agg", rows=R.n, groups=len(groups)))
        keys = list(groups)
        cols = [np.array([k[j] for k in keys], dtype=np.int64) for j in range(len(node["groups"]))]
        valid = [None if all(k[j] is not None for k in keys) else np.array([k[j] is not None for k in keys]) for j in range(len(node["groups"]))]
        kinds = [R.kinds[g] for g in node["groups"]]
        for a, (kind, c) in enumerate(node["aggs"]):
            assert kind != "avg"
            # count(x) over no non-NULL input finalises to NULL here, as in the engine this library stands in for (planhip.h, PH_JT_LEFT: "count(x)
            # of a customer without orders is 0 and finalises to NULL"): at the root that is a count of 0, below other operators a NULL
            vals = [None if kind == "count" and groups[k][a] == 0 else groups[k][a] for k in keys]
            ok = np.array([v is not None for v in vals], dtype=bool)
            cols.append(np.array([0 if v is None else v for v in vals], dtype=np.int64))
            valid.append(None if ok.all() else ok)
            kinds.append(("dec", 0 if kind in ("count", "count_star", "count_distinct") else R.kinds[c][1]))
        return Rel(cols, valid, kinds, None)
    P, B = _eval(node["probe"], tables, trace), _eval(node["build"], tables, trace)
    pk, bk = [P.cols[c] for c in node["pkeys"]], [B.cols[c] for c in node["bkeys"]]
    res = None
    if node["residual"]:
        a, op, b = node["residual"]

        def side(c, pr, br):
            return P.cols[c][pr] if c < len(P.cols) else B.cols[c - len(P.cols)][br]
        res = lambda pr, br: ref_filter(side(a, pr, br), op, side(b, pr, br))   # noqa: E731
    ipr, ibr = ref_join("inner", pk, bk, res)
    per_probe = np.bincount(ipr, minlength=max(P.n, 1)) if len(ipr) else np.zeros(1, dtype=np.int64)
    trace.append(dict(op="join", kind=node["kind"], probe=P.n, build=B.n, pairs=len(ipr), matched=int((per_probe > 0).sum()), max_fan=int(per_probe.max())))
    kinds = P.kinds + B.kinds
    if node["kind"] in ("semi", "anti"):
        rows = ref_join(node["kind"], pk, bk, res)
        cols, valid = P.take(rows)
        rid = None if P.rid is None else P.rid[rows]
        assert all(o < len(P.cols) for o in node["out"])
    else:
        pr, br = (ipr, ibr) if node["kind"] == "inner" else ref_join("left", pk, bk, res)
        pc, pv = P.take(pr)
        bc, bv = B.take(br, null=(br < 0) if node["kind"] == "left" else None)
        cols, valid = pc + bc, pv + bv
        rid = None if P.rid is None else P.rid[pr]
    return Rel([cols[o] for o in node["out"]], [valid[o] for o in node["out"]], [kinds[o] for o in node["out"]], rid)


def ref_plan(root, tables):
    """the plan's result as the device tests compare it, and the facts that make the case a test.
    A join-rooted plan: ("rows", sorted row tuples, [(typ, scale) per column]); an aggregate-rooted one: ("groups", {key tuple: [aggregate
    results]}, [scale of each aggregate's argument, None for count(*)]).
    facts: total = rows of the plan's leftmost table, kept = how many of them reach the root (its aggregate's input), out = rows / groups of the
    result, joins = the trace entries of the joins in evaluation order."""
    trace = []
    if root["op"] == "agg":
        R = _eval(root["child"], tables, trace)
        groups = _groups_of(root, R)
        result = ("groups", groups, [None if c is None else R.kinds[c][1] for _, c in root["aggs"]])
        nout = len(groups)
    else:
        R = _eval(root, tables, trace)
        assert all(v is None for v in R.valid), "fetch_rows returns no NULL-able column"
        rows = sorted(zip(*[[x if isinstance(x, bytes) else int(x) for x in c] for c in R.cols])) if R.n else []
        result = ("rows", rows, R.kinds)
        nout = R.n
    first = next(t for t in trace if t["op"] == "scan")
    facts = dict(total=first["rows"], kept=R.n if R.rid is None else len(np.unique(R.rid)), out=nout, input=R.n,
                 joins=[t for t in trace if t["op"] == "join"], scans=[t for t in trace if t["op"] == "scan"])
    return result, facts




# ------------------------------------------------------------------ the cases
# explain() phrases that name a form
LOOK, MERGE, RUN, COUNTED = "strict N:1 lookup", "merge lookup", "run lookup", "counted N:1 lookup"
CONS, MISSCOMP = "conservative forms", "compaction of the misses"
FUSEDBUILD, GATED, SELROWS, INTER = "filter fused into the direct build", "gated sorted fill", "build: selected rows", "build: intermediate rows"
FPROBE, PROBE = "probe: fused filter+probe,", "probe: probe,"
SEMI, ANTI = "probe: semi (marks + selection)", "probe: anti (marks + selection)"
MARKS1, LATE = "filter + semi-join marks in one pass", "evaluated BEHIND the join"
RESID, SEMIRES, ANTIRES = "residual condition over the pairs", "SEMI with a residual condition", "ANTI with a residual condition"
LEFT, CHILDREN, KEYPUSH = "LEFT OUTER", "children per parent", "input reduced to the rows the keys of join#"
GROUPSDEV, STREAM, HASH = "groups stay on the device as a relation", "streaming aggregate", "hash aggregate"
SIDEWAYS, SWAP, NOTABLE = "build side reduced by the probe key's domain", "roles swapped", "no table — the build side is clustered"
FUSEDSCAN, DISTINCT = "fused scan plan", "count(distinct)"
TOOMANY, NOWORD = "group keys do not fit the aggregate table's four key words", "count(distinct) needs a key word"
SEMIPAIRS, ANTIPAIRS = "SEMI through the pairs of the table-less join", "ANTI through the pairs of the table-less join"

NFACT, NDIM = 70_001, 4099                   # ragged against 256, 1024 and 4096
VARIANTS = ("base", "probe_empty", "build_empty", "all_miss", "one_row", "global", "global_empty")


class V:
    """one degenerate shape of a form: what it does to the form's tables and plan"""

    def __init__(self, name):
        assert name in VARIANTS, name
        self.name = name
        self.one = name == "one_row"
        self.glob = name in ("global", "global_empty")
        self.dang = "all" if name == "all_miss" else None
        self.nf, self.nd = (1, 1) if self.one else (NFACT, NDIM)
        self.probe_empty = name in ("probe_empty", "global_empty")
        self.build_empty = name == "build_empty"

    def pe(self, col, preds=(), replace=False, twice=False):
        """the probe scan's conjuncts: the form's own, and for the emptied probe side one that no row passes (col holds 0..99 / row numbers).
        Where the NUMBER of conjuncts picks the form, the emptying one replaces the form's first (replace), or comes twice (twice: two
        conjuncts never ride in the probe)"""
        if not self.probe_empty:
            return list(preds)
        return [(col, "lt", 0)] + list(preds)[1:] if replace else list(preds) + [(col, "lt", 0)] * (2 if twice else 1)

    def be(self, col, preds=()):
        """the build scan's conjuncts; an emptied build side REPLACES the first of the form's own (the number of conjuncts picks the form)"""
        return ([(col, "lt", 0)] + list(preds)[1:]) if self.build_empty else list(preds)

    def d(self, some="none"):
        return self.dang or some


CASES = {}


def _global_aggs(c):
    return [("count_star", None), ("count", c), ("sum", c), ("min", c), ("max", c), ("avg", c)]


def _add(form, v, tables, plan, phrases, gcol=None, absent=(), env=(), label=None, point=None, error=None, name=None, variant=None, codes=None):
    """register one case. v: a V (the plan is wrapped in the global aggregate over column gcol for its two global variants) or None.
    label: what the CPU test checks of the case's inputs — "ordinary" 0 < kept < total, "empty" kept == 0, "all" every row that passes the probe
    scan is kept, "any" nothing (one-row tables). point: "misses" / "dups" — a join of the plan has probe rows without a partner / a probe row
    with more than 16; "childless" / "childless+several" — every parent of the LEFT join has no child / some have none and some more than one.
    codes: (group key, "rows" or "interned") — what the fetched values of that VARCHAR group key are: the group's own row (one per group) or
    the first row that holds the string (one per different string). The explain text names neither, so this is what witnesses the form."""
    vn = variant or (v.name if v is not None else "base")
    if v is not None and v.glob:
        assert gcol is not None
        plan = agg(plan, [], _global_aggs(gcol))
        phrases = tuple(phrases) + (HASH,)
    name = name or (form if vn == "base" else f"{form}-{vn}")
    assert name not in CASES, name
    CASES[name] = dict(name=name, form=form, variant=vn, tables=tables, plan=plan, phrases=tuple(phrases), absent=tuple(absent), env=tuple(env),
                       label=label, point=point, error=error, codes=codes)


def _label(v, kind="inner"):
    if v.one:
        return "any"
    if v.probe_empty:
        return "empty"
    if v.build_empty or v.dang:
        return "all" if kind in ("anti", "left") else "empty"
    return "ordinary"


INNER_OUT = [F_KEY, F_AMT, F_ID, NF + DIM_PAY, NF + DIM_ATTR]
PROBE_OUT = [F_KEY, F_AMT, F_ID]


def _lookups():
    # strict N:1 lookup: fact(shuffled) against the unfiltered dim whose payload is used above. Keys: an int32 range that starts at INT32_MIN.
    # A one-row probe side is ordered, so one row against one row is a merge lookup.
    for vn in VARIANTS:
        v = V(vn)
        d = dim(v.nd, "i32_min")
        f = fact(v.nf, d, "shuffled", v.d())
        plan = join(scan("f", v.pe(F_X, [(F_X, "lt", 50)])), scan("d", v.be(DIM_ATTR)), [F_KEY], [DIM_KEY], INNER_OUT)
        ph = {"build_empty": (GATED,), "all_miss": (CONS, COUNTED, MISSCOMP), "one_row": (MERGE,)}.get(vn, (LOOK,))
        # (a filtered build side never takes a lookup: the build-emptied shape is a case of the gated fill, under that name)
        _add("gated" if v.build_empty else "lookup", v, dict(f=f, d=d), plan, ph, gcol=3, label=_label(v), point="misses" if v.dang else None,
             name="gated-build_empty-under-filtered-probe-i32_min" if v.build_empty else None)
    # merge lookup: fact(ascending) against the unfiltered dim with its strict key. Keys: an int64 range that ends at INT64_MAX.
    for vn in VARIANTS:
        v = V(vn)
        d = dim(v.nd, "i64_max")
        f = fact(v.nf, d, "ascending", v.d())
        plan = join(scan("f", v.pe(F_X, [(F_X, "lt", 50)])), scan("d", v.be(DIM_ATTR)), [F_KEY], [DIM_KEY], INNER_OUT)
        ph = {"build_empty": (GATED,), "all_miss": (MERGE, CONS, COUNTED, MISSCOMP)}.get(vn, (MERGE,))
        _add("gated" if v.build_empty else "merge", v, dict(f=f, d=d), plan, ph, gcol=3, label=_label(v), point="misses" if v.dang else None,
             name="gated-build_empty-under-ordered-probe-i64_max" if v.build_empty else None)
        if vn == "base":
            _add("merge", None, dict(f=f, d=d), plan, (LOOK,), absent=(MERGE,), env=("PH_PLAN_NO_MERGE",), label="ordinary", name="merge-NO_MERGE")
    # run lookup: a two-key join into runs(), declared unique on both columns (a one-row table has no runs: no such variant)
    for run_len in (3, 4):
        for vn in VARIANTS:
            if vn == "one_row" or (run_len == 3 and vn != "base"):
                continue
            v = V(vn)
            r = runs(1367 if run_len == 3 else 1025, run_len)
            f = fact2(v.nf, r, v.d())
            plan = join(scan("f", v.pe(F2_X, [(F2_X, "lt", 50)])), scan("r", v.be(R_K2)), [F2_K1, F2_K2], [R_K1, R_K2], [F2_K1, F2_K2, F2_AMT, F2_ID, NF2 + R_PAY])
            ph = {"build_empty": (SELROWS,), "all_miss": (RUN, CONS, COUNTED, MISSCOMP)}.get(vn, (RUN,))
            _add("selrows" if v.build_empty else f"run{run_len}", v, dict(f=f, r=r), plan, ph, gcol=4, label=_label(v), point="misses" if v.dang else None,
                 name="selrows-build_empty-two-keys" if v.build_empty else None)
            if vn == "base":
                _add(f"run{run_len}", None, dict(f=f, r=r), plan, (LOOK,), absent=(RUN,), env=("PH_PLAN_NO_RUN_LOOKUP",), label="ordinary", name=f"run{run_len}-NO_RUN_LOOKUP")
    # counted N:1 lookup + conservative: the three lookup forms with SOME dangling foreign keys (all of them dangle in the all_miss variants above)
    d = dim(NDIM, "i32_max")
    _add("counted-lookup", None, dict(f=fact(NFACT, d, "shuffled", "some"), d=d), join(scan("f"), scan("d"), [F_KEY], [DIM_KEY], INNER_OUT),
         (LOOK, CONS, COUNTED, MISSCOMP), label="ordinary", point="misses")
    d = dim(NDIM, "i64_sparse")
    _add("counted-merge", None, dict(f=fact(NFACT, d, "ascending", "some"), d=d), join(scan("f"), scan("d"), [F_KEY], [DIM_KEY], INNER_OUT),
         (MERGE, CONS, COUNTED, MISSCOMP), label="ordinary", point="misses")
    r = runs(1025, 4)
    _add("counted-run", None, dict(f=fact2(NFACT, r, "some"), r=r), join(scan("f"), scan("r"), [F2_K1, F2_K2], [R_K1, R_K2], [F2_K1, F2_K2, F2_AMT, F2_ID, NF2 + R_PAY]),
         (RUN, CONS, COUNTED, MISSCOMP), label="ordinary", point="misses")
    # a build key that is declared unique but is not: the lookup meets two build rows for one key and says so (ph_table_declare_unique)
    dd = dupdim(255, "i32_mid")
    dd["unique"] = [[0]]
    _add("declared-unique-has-duplicates", None, dict(f=fact(NDIM, dd, "shuffled"), d=dd), join(scan("f"), scan("d"), [F_KEY], [0], [F_KEY, F_ID, NF + 1]),
         (), label="any", point="dups", error=("PH_ECONSTRAINT", "declared unique has duplicates"))
    # the four key-domain placements and the ordinary row counts, through the lookup (every fifth key dangles: counted, conservative)
    for place in ("i32_min", "i32_max", "i64_sparse", "i64_max"):
        for nf, nd in ((255, 255), (4099, 255), (NFACT, NDIM)):
            d = dim(nd, place)
            _add("placement", None, dict(f=fact(nf, d, "shuffled", "some"), d=d), join(scan("f"), scan("d"), [F_KEY], [DIM_KEY], INNER_OUT),
                 (LOOK, CONS, COUNTED), label="ordinary", point="misses", name=f"placement-lookup-{place}-{nf}x{nd}")


def _builds():
    # one pushed conjunct under the build scan: fused into the direct build (dense key, stored out of order) / the gated sorted fill (strict key)
    for form, shuffle, phrase in (("fusedbuild", True, FUSEDBUILD), ("gated", False, GATED)):
        for vn in VARIANTS:
            if vn == "one_row" and shuffle:
                continue                     # (a one-row key is strict: the gated fill's case)
            v = V(vn)
            d = dim(v.nd, "i32_max", shuffle=shuffle)
            f = fact(v.nf, d, "shuffled", v.d())
            plan = join(scan("f", v.pe(F_X)), scan("d", v.be(DIM_ATTR, [(DIM_ATTR, "ge", 2)])), [F_KEY], [DIM_KEY], INNER_OUT)
            _add(form, v, dict(f=f, d=d), plan, (phrase,), gcol=3, label=_label(v), point=None if v.one or v.probe_empty else "misses")
    # two conjuncts under the build scan: the table over the selected rows
    for vn in VARIANTS:
        if vn == "one_row":
            continue
        v = V(vn)
        d = dim(v.nd, "i32_min")
        f = fact(v.nf, d, "shuffled", v.d())
        plan = join(scan("f", v.pe(F_X)), scan("d", v.be(DIM_ATTR, [(DIM_ATTR, "ge", 2), (DIM_PAY, "gt", -500_000)])), [F_KEY], [DIM_KEY], INNER_OUT)
        _add("selrows", v, dict(f=f, d=d), plan, (SELROWS,), gcol=3, label=_label(v), point=None if v.probe_empty else "misses")
    # the build side is itself a join's output (dim x tiny on attr: two lanes): the table over intermediate rows
    for vn in VARIANTS:
        v = V(vn)
        d = dim(v.nd, "i64_sparse")
        f = fact(v.nf, d, "shuffled", v.d())
        t = tiny((3,)) if v.one else tiny()
        inner = join(scan("d"), scan("t", v.be(0, [(0, "ge", 2)])), [DIM_ATTR], [0], [DIM_KEY, DIM_PAY, ND + 1])
        plan = join(scan("f", v.pe(F_X)), inner, [F_KEY], [0], [F_KEY, F_AMT, F_ID, NF + 1, NF + 2])
        _add("intermediate", v, dict(f=f, d=d, t=t), plan, (INTER,), gcol=3, label=_label(v), point=None if v.one or v.probe_empty else "misses")


def _pairs():
    # N:M: dupdim with fan-out 1 / 2 / 17; one conjunct on the probe scan rides in the probe, none leaves the plain probe
    for form, preds in (("fprobe", [(F_X, "lt", 50)]), ("probe", [])):
        for vn in VARIANTS:
            if vn == "one_row" and form == "fprobe":
                continue
            v = V(vn)
            d = dupdim(1 if v.one else 255, "i32_max")
            f = fact(v.nf if v.one else NDIM, d, "shuffled", v.d("some"))
            # (the emptied probe side keeps the form's number of conjuncts: one rides in the probe, none or two do not)
            plan = join(scan("f", v.pe(F_X, preds, replace=form == "fprobe", twice=form == "probe")), scan("d", v.be(2)), [F_KEY], [0], [F_KEY, F_AMT, F_ID, NF + 1, NF + 2])
            ph = (MERGE,) if v.one else (FPROBE,) if form == "fprobe" else (PROBE,)
            _add(form, v, dict(f=f, d=d), plan, ph, gcol=3, label=_label(v), point="dups" if vn in ("base", "global") else None)
    # SEMI against duplicate build keys and ANTI: marks + selection. One row against one row: the key is unique, the SEMI join a plain probe.
    for kind, phrase in (("semi", SEMI), ("anti", ANTI)):
        for vn in VARIANTS:
            v = V(vn)
            d = dupdim(1 if v.one else 255, "i64_max")
            f = fact(v.nf if v.one else NDIM, d, "shuffled", v.d("some"))
            plan = join(scan("f", v.pe(F_X)), scan("d", v.be(2)), [F_KEY], [0], PROBE_OUT, kind=kind)
            ph = (PROBE,) if v.one and kind == "semi" else (phrase,)
            _add(kind, v, dict(f=f, d=d), plan, ph, gcol=1, label="any" if v.one else _label(v, kind), point="misses" if vn == "base" else None)
    # a SEMI join whose result is the build child of a second join: filter + marks in one pass, the marks ride in the second build
    for vn in VARIANTS:
        v = V(vn)
        d = dim(v.nd, "i32_min")
        keep = dupdim(1 if v.one else NDIM // 3, "i32_min", fan=(1, 2))     # the first third of dim's keys, some twice
        f = fact(v.nf, d, "shuffled", v.d())
        inner = join(scan("d", v.be(DIM_ATTR, [(DIM_ATTR, "ge", 1)])), scan("k"), [DIM_KEY], [0], [DIM_KEY, DIM_PAY, DIM_ATTR], kind="semi")
        plan = join(scan("f", v.pe(F_X)), inner, [F_KEY], [0], [F_KEY, F_AMT, F_ID, NF + 1, NF + 2])
        _add("marks-for-build", v, dict(f=f, d=d, k=keep), plan, (MARKS1,), gcol=3, label=_label(v), point=None if v.one or v.probe_empty else "misses")
    # residual conditions: INNER over the pairs, SEMI and ANTI through marks of the pairs that keep it (x <= z, both 0..99)
    for kind, phrase in (("inner", RESID), ("semi", SEMIRES), ("anti", ANTIRES)):
        for vn in VARIANTS:
            v = V(vn)
            d = dupdim(1 if v.one else 255, "i32_mid")
            f = fact(v.nf if v.one else NDIM, d, "shuffled", v.d("some"))
            out = [F_KEY, F_X, F_ID, NF + 1, NF + 3] if kind == "inner" else PROBE_OUT
            plan = join(scan("f", v.pe(F_X)), scan("d", v.be(2)), [F_KEY], [0], out, kind=kind, residual=(F_X, "le", NF + 3))
            _add(f"residual-{kind}", v, dict(f=f, d=d), plan, (phrase,), gcol=3 if kind == "inner" else 1,
                 label="any" if v.one else _label(v, kind), point="dups" if vn == "base" else None)


def _outer():
    # LEFT OUTER: count(build column) and count(*) per probe key, sum / min / max / avg of the build payload (NULL where there is no match)
    for vn in VARIANTS:
        v = V(vn)
        d = dupdim(1 if v.one else 255, "i32_min")
        f = fact(v.nf if v.one else NDIM, d, "shuffled", v.d("some"))
        j = join(scan("f", v.pe(F_X)), scan("d", v.be(2)), [F_KEY], [0], [F_KEY, NF + 1], kind="left")
        aggs = [("count", 1), ("count_star", None), ("sum", 1), ("min", 1), ("max", 1), ("avg", 1)]
        plan = agg(j, [] if v.glob else [0], aggs)
        _add("left", None, dict(f=f, d=d), plan, (LEFT, HASH), label="any" if v.one else "empty" if v.probe_empty else "all", point="misses" if vn == "base" else None,
             name="left" if vn == "base" else f"left-{vn}", variant=vn)
    # children per parent: Agg(count(child column)) <- LEFT JOIN(parent with a unique key, child), the counts grouped again above (Q13's shape:
    # how many parents have 0 (NULL), 1, 2 ... children, and which). Without one group key the shape is a plain LEFT OUTER join.
    for vn in VARIANTS:
        v = V(vn)
        d = dim(1 if v.one else 255, "i32_max")
        f = fact(v.nf if v.one else NDIM, d, "shuffled", v.d("some"))
        j = join(scan("d", v.pe(DIM_ATTR)), scan("f", v.be(F_X)), [DIM_KEY], [F_KEY], [DIM_KEY, ND + F_AMT, ND + F_ID], kind="left")
        inner = agg(j, [] if v.glob else [0], [("count", 1), ("count", 2)])
        off = 0 if v.glob else 1
        plan = agg(inner, [off], [("count_star", None), ("count", off + 1), ("sum", off + 1)] + ([] if v.glob else [("min", 0), ("max", 0), ("sum", 0)]))
        ph = (LEFT, GROUPSDEV) if v.glob else (CHILDREN,)
        label = "empty" if vn == "probe_empty" else "any"
        point = "childless+several" if vn in ("base", "global") else "childless" if vn in ("build_empty", "all_miss") else None
        _add("children", None, dict(d=d, f=f), plan, ph, label=label, point=point, name="children" if vn == "base" else f"children-{vn}", variant=vn)
        if vn == "base":
            _add("children", None, dict(d=d, f=f), plan, (LEFT, GROUPSDEV), absent=(CHILDREN,), env=("PH_PLAN_NO_COUNT_PUSHDOWN",), label="any", point="childless+several", name="children-NO_COUNT_PUSHDOWN")


def _aggregates():
    # an aggregate below a join: its groups stay on the device as a relation
    for vn in VARIANTS:
        v = V(vn)
        d = dim(1 if v.one else 255, "i64_max")
        f = fact(v.nf if v.one else NDIM, d, "shuffled", v.d("some"))
        below = agg(scan("f", v.be(F_X)), [F_KEY], [("sum", F_AMT), ("count_star", None)])
        plan = join(scan("d", v.pe(DIM_ATTR, [(DIM_ATTR, "ge", 1)])), below, [DIM_KEY], [0], [DIM_KEY, DIM_PAY, ND + 1, ND + 2])
        _add("groups-below", v, dict(d=d, f=f), plan, (GROUPSDEV, INTER), gcol=2, label=_label(v), point=None)
    # the root aggregate: streaming over rows ordered by the first key, hashed otherwise, hashed for one global group. No input row: the
    # streaming aggregate is not entered.
    for form, order in (("stream", "ascending"), ("hash", "shuffled")):
        for vn in VARIANTS:
            if vn in ("global", "global_empty") and form == "hash":
                continue
            v = V(vn)
            d = dim(v.nd, "i32_min")
            f = fact(v.nf, d, order, v.d())
            j = join(scan("f", v.pe(F_X, [(F_X, "lt", 50)])), scan("d", v.be(DIM_ATTR)), [F_KEY], [DIM_KEY], [F_KEY, F_AMT, NF + DIM_PAY])
            aggs = [("count_star", None), ("count", 1), ("sum", 1), ("min", 2), ("max", 2), ("avg", 2)]
            plan = agg(j, [] if v.glob else [0], aggs)
            streams = (form == "stream" and vn == "base") or v.one           # (one row is ordered)
            ph = (STREAM,) if streams else (HASH,)
            # (every probe row missing: the optimistic run streams its rows before the strict lookup's misses surface, the conservative rerun hashes)
            _add(form, None, dict(f=f, d=d), plan, ph, absent=() if streams or v.dang else (STREAM,), label=_label(v), name=form if vn == "base" else f"{form}-{vn}", variant=vn)
            if vn == "base" and form == "stream":
                _add(form, None, dict(f=f, d=d), plan, (HASH,), absent=(STREAM,), env=("PH_PLAN_NO_STREAM_AGG",), label="ordinary", name="stream-NO_STREAM_AGG")


def _scan_aggregates():
    # Agg <- Scan at the root runs as a fused scan plan, which reports the groups some row reached: the aggregate without GROUP BY has its one
    # group there too when the scan's filter passes no row — the answer does not depend on the lowering
    d = dim(NDIM, "i32_mid")
    f = fact(NFACT, d, "shuffled")
    for vn, label, preds in (("global", "ordinary", [(F_X, "lt", 50)]), ("global_empty", "empty", [(F_X, "lt", 0)])):
        _add("scan-agg", None, dict(f=f), agg(scan("f", preds), [], _global_aggs(F_AMT)), (FUSEDSCAN,), label=label, name=f"scan-agg-{vn}", variant=vn)


def _chains():
    # sideways information passing: fact x small filtered dim, then the same key against a big (>= 2^18 rows) table, which is first reduced to
    # the rows the small table's surviving keys can reach
    nbig = (1 << 18) + 3
    for vn in VARIANTS:
        if vn == "one_row":
            continue
        v = V(vn)
        s, b = dim(NDIM, "i32_mid"), dim(nbig, "i32_mid")
        f = fact(NFACT, s, "shuffled", v.d())
        j1 = join(scan("f", v.pe(F_X)), scan("s", v.be(DIM_ATTR, [(DIM_ATTR, "ge", 2)])), [F_KEY], [DIM_KEY], [F_KEY, F_AMT, F_ID, NF + DIM_PAY])
        plan = join(j1, scan("b"), [0], [DIM_KEY], [0, 1, 2, 3, 4 + DIM_PAY])
        _add("sideways", v, dict(f=f, s=s, b=b), plan, (SIDEWAYS,), gcol=4, label=_label(v), point=None)
    # a three-join chain whose second join is empty: everything above it sees 0 rows
    d, t = dim(NDIM, "i32_min"), tiny()
    f = fact(NFACT, d, "shuffled")
    j1 = join(scan("f"), scan("d"), [F_KEY], [DIM_KEY], [F_KEY, F_ID, F_Y, NF + DIM_ATTR])
    j2 = join(j1, scan("t", [(0, "gt", 100)]), [3], [0], [0, 1, 2, 4 + 1])
    plan = join(j2, scan("t2"), [2], [0], [0, 1, 2, 3, 4 + 1])
    _add("chain-empty-second-join", None, dict(f=f, d=d, t=t, t2=tiny(tuple(range(0, 100, 3)))), plan, (LOOK,), label="empty")
    # an N:M join, then an N:1 lookup whose probe side is that intermediate (the key comes from the first join's build side)
    dd = dupdim(255, "i64_sparse")
    f = fact(NDIM, dd, "shuffled", "some")
    j1 = join(scan("f"), scan("d"), [F_KEY], [0], [F_KEY, F_ID, NF + 1, NF + 2])
    plan = join(j1, scan("t"), [3], [0], [0, 1, 2, 3, 4 + 1])
    _add("chain-pairs-then-lookup", None, dict(f=f, d=dd, t=tiny()), plan, (PROBE, LOOK), label="ordinary", point="dups")
    # VARCHAR key pair: an empty string, a byte >= 0x80, a proper prefix of another string, a probe string the build side does not have
    bs = strings([b"", b"caf\xc3\xa9", b"ab", b"abc", b"abc", b"zz"])
    ps = strings([b"abc", b"", b"ab", b"absent", b"caf\xc3\xa9", b"a", b"caf", b"ab"] * 33)
    tb = T([C("str", bs), C("dec", np.arange(len(bs)) * 101 - 200, 2)])
    tp = T([C("str", ps), C("i32", np.arange(len(ps)))])
    _add("string-keys", None, dict(p=tp, b=tb), join(scan("p"), scan("b"), [0], [0], [0, 1, 2 + 1]), (PROBE,), label="ordinary", point="misses")


def _clustered():
    big = clustered()
    nk = big["nkeys"]
    # small sides against the clustered table: NDIM keys spread over its key range and beyond it (every key past nk dangles)
    step = nk // (NDIM - 400)
    small = dim(NDIM, "i32_mid")
    small["cols"][DIM_KEY] = C("i32", np.arange(NDIM, dtype=np.int64) * step)
    tabs = dict(big=big, s=small)
    bout = [BIG_KEY, BIG_A, BIG_ID, NBIG + DIM_PAY]
    # roles swapped: the clustered table probes a (filtered) handful of rows
    plan = join(scan("big"), scan("s", [(DIM_ATTR, "ge", 2)]), [BIG_KEY], [DIM_KEY], bout)
    _add("swap", None, tabs, plan, (SWAP, NOTABLE), label="ordinary", point="misses")
    _add("swap", None, tabs, plan, (PROBE,), absent=(SWAP, NOTABLE), env=("PH_PLAN_NO_SWAP",), label="ordinary", name="swap-NO_SWAP")
    _add("swap", None, tabs, plan, (PROBE,), absent=(SWAP, NOTABLE), env=("PH_PLAN_NO_SORTED_PAIRS",), label="ordinary", name="swap-NO_SORTED_PAIRS")
    # no table: the small side probes the clustered table, whose own filter is applied to the pairs
    sout = [DIM_KEY, DIM_PAY, ND + BIG_A, ND + BIG_ID]
    plan = join(scan("s"), scan("big", [(BIG_A, "lt", 50)]), [DIM_KEY], [BIG_KEY], sout)
    _add("notable", None, tabs, plan, (NOTABLE, "filters applied to the pairs"), label="ordinary", point="dups")
    _add("notable", None, tabs, plan, (" pairs from ",), absent=(NOTABLE,), env=("PH_PLAN_NO_SORTED_PAIRS",), label="ordinary", name="notable-NO_SORTED_PAIRS")
    # SEMI / ANTI through the pairs of the table-less join
    for kind, phrase, fallback in (("semi", SEMIPAIRS, SEMI), ("anti", ANTIPAIRS, ANTI)):
        plan = join(scan("s"), scan("big"), [DIM_KEY], [BIG_KEY], [DIM_KEY, DIM_PAY, DIM_ATTR], kind=kind)
        _add(f"exists-pairs-{kind}", None, tabs, plan, (phrase, NOTABLE), label="ordinary", point="misses")
        _add(f"exists-pairs-{kind}", None, tabs, plan, (fallback,), absent=(phrase, NOTABLE), env=("PH_PLAN_NO_EXISTS_PAIRS",), label="ordinary",
             name=f"exists-pairs-{kind}-NO_EXISTS_PAIRS")
    # the probe scan's column-vs-column conjunct evaluated behind a selective N:1 join (the probe table must have 2^22 rows for it: the clustered one)
    for vn in VARIANTS:
        if vn == "one_row":
            continue
        v = V(vn)
        s = small
        if v.dang:
            s = dim(NDIM, "i32_mid")
            s["cols"][DIM_KEY] = C("i32", nk + 5 + np.arange(NDIM, dtype=np.int64) * 3)
        plan = join(scan("big", v.pe(BIG_A), colcmp=(BIG_A, "lt", BIG_B)), scan("s", v.be(DIM_ATTR)), [BIG_KEY], [DIM_KEY], bout)
        _add("late-filter", v, dict(big=big, s=s), plan, (LATE,), gcol=3, label=_label(v), point=None)
        if vn == "base":
            _add("late-filter", None, dict(big=big, s=s), plan, (SWAP, NOTABLE, "filters applied to the pairs"), absent=(LATE,), env=("PH_PLAN_NO_LATE_FILTER",), label="ordinary", name="late-filter-NO_LATE_FILTER")
    # the probe side's keys go down into a build-side aggregate grouped by the join key (its input must have 2^20 rows: the clustered table)
    for kind in ("inner", "semi"):
        for vn in VARIANTS:
            if vn == "one_row" or (kind == "semi" and vn != "base"):
                continue
            v = V(vn)
            s = small
            if v.dang:
                s = dim(NDIM, "i32_mid")
                s["cols"][DIM_KEY] = C("i32", nk + 5 + np.arange(NDIM, dtype=np.int64) * 3)
            below = agg(scan("big", v.be(BIG_A)), [BIG_KEY], [("sum", BIG_A), ("count_star", None), ("min", BIG_ID), ("max", BIG_ID)])
            out = [DIM_KEY, DIM_PAY, ND + 1, ND + 2, ND + 3, ND + 4] if kind == "inner" else [DIM_KEY, DIM_PAY, DIM_ATTR]
            plan = join(scan("s", v.pe(DIM_ATTR, [(DIM_ATTR, "ge", 1)])), below, [DIM_KEY], [0], out, kind=kind)
            _add(f"key-pushdown-{kind}", v, dict(s=s, big=big), plan, (KEYPUSH, GROUPSDEV), gcol=1, label=_label(v), point=None)
            if vn == "base":
                _add(f"key-pushdown-{kind}", None, dict(s=s, big=big), plan, (GROUPSDEV,), absent=(KEYPUSH,), env=("PH_PLAN_NO_KEY_PUSHDOWN",), label="ordinary",
                     name=f"key-pushdown-{kind}-NO_KEY_PUSHDOWN")


EDGE4 = (I32_MIN, -1, 0, I32_MAX)
K_HI, K_DATE, K_HI2, K_CODE, K_FIFTH, K_SEL, K_AMT, K_ID, K_X, K_Y, NK = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10


def keyed(n=NDIM):
    """six group-key columns whose 512 combinations repeat every 512 rows: hi INTEGER and date DATE run through INT32_MIN, -1, 0, INT32_MAX
    against each other (the two halves of one packed word), hi2 INTEGER the same against code (a dictionary code), fifth INTEGER, sel INTEGER
    0..3 (a LEFT join against tiny((0, 1, 2)) makes a NULL-able key of it: a table's own NULL-able column cannot be materialised); amt
    DECIMAL(.., 2), id = the row number, x < y is a column-vs-column conjunct that keeps the plan off the fused scan"""
    i = np.arange(n, dtype=np.int64)
    j = i % 512
    e = np.array(EDGE4, dtype=np.int64)
    return T([C("i32", e[j % 4]), C("date", e[(j // 4) % 4]), C("i32", e[(j // 16) % 4]), C("code", (j // 64) % 2, dictionary=ATTR_DICT), C("i32", (j // 128) % 2 * 1000 - 500),
              C("i32", (j // 128) % 4), C("dec", (i * 48271) % 200_001 - 100_000, 2), C("i32", i), C("i32", (i * 37) % 100), C("i32", (i * 53) % 100)])


D_G, D_SEL, D_AMT, D_ID, D_W1, D_W2, D_W3, NDI = 0, 1, 2, 3, 4, 5, 6, 7
DISTINCT_ARGS = 11


def distinct_input(n=NDIM):
    """g INTEGER 0..36, sel INTEGER 0..12 (a LEFT join against distinct_args() makes the argument of it: a table's own NULL-able column cannot
    be materialised), amt DECIMAL(.., 2), id = the row number, w1..w3 BIGINT 0..1 (with g: four whole key words)"""
    i = np.arange(n, dtype=np.int64)
    return T([C("i32", i % 37), C("i32", (i * 7) % 13), C("dec", (i * 16807) % 50_001 - 25_000, 2), C("i32", i), C("i64", i % 2), C("i64", (i // 2) % 2), C("i64", (i // 4) % 2)])


def distinct_args():
    """key INTEGER 0..10 (unique), arg INTEGER key % 6 - 2: sel 11 and 12 find no row (a NULL argument), two keys share most arguments"""
    k = np.arange(DISTINCT_ARGS, dtype=np.int64)
    return T([C("i32", k), C("i32", k % 6 - 2)], unique=[[0]])


S_ID, S_STR, S_X, S_AMT, S_Y = 0, 1, 2, 3, 4
STRING_POOL = (b"", b"caf\xc3\xa9", b"ab", b"abc", b"zz", b"caf", b"\xff\x80", b"abcd", b"a")


def named(n=NDIM):
    """id INTEGER = the row number (strictly ascending, declared unique), s VARCHAR from a pool with an empty string, bytes >= 0x80 and proper
    prefixes of other strings, x and y INTEGER 0..99, amt DECIMAL(.., 2)"""
    i = np.arange(n, dtype=np.int64)
    return T([C("i32", i), C("str", strings([STRING_POOL[(int(k) * 5 + 2) % len(STRING_POOL)] for k in i])), C("i32", (i * 37) % 100), C("dec", (i * 69621) % 30_001 - 15_000, 2),
              C("i32", (i * 53) % 100)], unique=[[S_ID]])


def _agg_lowering():
    # more than four group keys at the root: two narrow NULL-free keys share a key word (high * 2^32 + low + 2^31), unpacked at the fetch
    t = keyed()
    aggs = [("count_star", None), ("sum", K_AMT), ("min", K_ID), ("max", K_ID)]
    # (the sixth key is the build key of a LEFT join: NULL where sel = 3 finds no partner)
    j = join(scan("t", [(K_X, "lt", 50)]), scan("n"), [K_SEL], [0], [K_HI, K_DATE, K_HI2, K_CODE, K_FIFTH, NK + 0, K_AMT, K_ID], kind="left")
    _add("packed-keys", None, dict(t=t, n=tiny((0, 1, 2))), agg(j, [0, 1, 2, 3, 4, 5], [("count_star", None), ("sum", 6), ("min", 7), ("max", 7)]), (HASH,),
         label="all")
    # (a plan takes at most eight group expressions: six narrow keys in three words and two DECIMALs in one each are five words)
    eight = [K_HI, K_DATE, K_HI2, K_CODE, K_FIFTH, K_SEL, K_AMT, K_AMT]
    _add("packed-keys", None, dict(t=t), agg(scan("t", colcmp=(K_X, "lt", K_Y)), eight, aggs), (), label="ordinary", error=("PH_EUNSUPPORTED", "8 " + TOOMANY),
         name="packed-keys-five-words")
    # ... but not below other operators: five keys are one too many there
    d = dim(NDIM, "i32_mid")
    below = agg(scan("t"), [K_ID, K_HI, K_DATE, K_HI2, K_FIFTH], [("count_star", None)])
    _add("packed-keys", None, dict(d=d, t=t), join(scan("d"), below, [DIM_KEY], [0], [DIM_KEY, ND + 5]), (), label="any", error=("PH_EUNSUPPORTED", "5 " + TOOMANY),
         name="packed-keys-five-below-a-join")
    # count(distinct): a side table keyed by (group keys, argument), beside a sum and a count(*) over the same rows
    tabs = dict(t=distinct_input(), a=distinct_args())
    aggs = [("count_distinct", 1), ("sum", 1), ("count_star", None), ("count", 1)]

    def with_arg(limit):                            # [g, arg (NULL where sel finds no row), w1, w2, w3]
        return join(scan("t", [(D_ID, "lt", limit)]), scan("a"), [D_SEL], [0], [D_G, NDI + 1, D_W1, D_W2, D_W3], kind="left")
    for vn, groups in (("base", [0]), ("global", [])):
        for empty in (False, True):
            name = "distinct" + ("" if vn == "base" else "-global") + ("-empty" if empty else "")
            _add("distinct", None, tabs, agg(with_arg(0 if empty else 3000), groups, aggs), (HASH,) if empty else (DISTINCT, HASH),
                 label="empty" if empty else "ordinary", name=name, variant="global_empty" if vn == "global" and empty else vn)
    _add("distinct", None, tabs, agg(with_arg(3000), [0, 2, 3, 4], aggs), (), label="ordinary", error=("PH_EUNSUPPORTED", NOWORD), name="distinct-no-key-word-left")
    # a VARCHAR group key: with the table's unique key among the group keys a group is one table row and its row id the string's code; else
    # (or with the switch) the strings are interned
    t = named()
    aggs = [("count_star", None), ("sum", S_AMT), ("max", S_X)]
    # (x < y keeps the plans off the fused scan, which takes no VARCHAR group column)
    plan = agg(scan("t", colcmp=(S_X, "lt", S_Y)), [S_ID, S_STR], aggs)
    both = " rows, 2 keys, 3 aggregates"
    _add("string-group-key", None, dict(t=t), plan, (both,), label="ordinary", codes=(1, "rows"))
    _add("string-group-key", None, dict(t=t), plan, (both,), env=("PH_PLAN_NO_ROW_CODES",), label="ordinary", codes=(1, "interned"), name="string-group-key-NO_ROW_CODES")
    _add("string-group-key", None, dict(t=t), agg(scan("t", colcmp=(S_X, "lt", S_Y)), [S_STR], aggs + [("min", S_ID)]), (HASH,), label="ordinary", codes=(0, "interned"),
         name="string-group-key-interned")
    # children per parent is no form for a LEFT join with a residual condition: the counts would ignore it
    d = dim(255, "i32_max")
    f = fact(NDIM, d, "shuffled", "some")
    j = join(scan("d"), scan("f"), [DIM_KEY], [F_KEY], [DIM_KEY, ND + F_AMT, ND + F_ID], kind="left", residual=(DIM_ATTR, "lt", ND + F_X))
    inner = agg(j, [0], [("count", 1), ("count", 2)])
    _add("children", None, dict(d=d, f=f), agg(inner, [1], [("count_star", None), ("count", 2), ("sum", 2), ("min", 0), ("max", 0), ("sum", 0)]), (), label="any",
         error=("PH_EUNSUPPORTED", "a LEFT join with a residual condition"), name="children-residual")


for _f in (_lookups, _builds, _pairs, _outer, _aggregates, _scan_aggregates, _chains, _agg_lowering):
    _f()
SMALL_CASES = tuple(CASES)
_clustered()
BIG_CASES = tuple(n for n in CASES if n not in SMALL_CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(result, facts) of a case, computed once and shared by the tests that need it"""
    c = CASES[name]
    return ref_plan(c["plan"], c["tables"])
