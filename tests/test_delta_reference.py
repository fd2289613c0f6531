"""Delta-encoded pages of the Parquet load path (PH_PARQUET_DELTA), without a GPU. The raw host decoder (ph_delta_decode_host, the host
instance of the __host__ __device__ functions the page kernels share) against the spec-restating decoder of tests/delta_cases.py on crafted
streams, valid and refused; ph_parquet_read_column_host_ex with the flag against pq.read_table value by value on pyarrow-written files
(DELTA_BINARY_PACKED integers, dates and integer-stored decimals, DELTA_LENGTH_BYTE_ARRAY strings; v1 / v2 pages, 37 rows a page, three row
groups, SNAPPY with flags 5); the type overrides; the refusals with and without the flag; one-byte patches; and all of it once more in a
stand-alone program under AddressSanitizer. Integers and bytes: equality is the tolerance."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

import delta_cases as D  # noqa: E402
import parquet_cases as C  # noqa: E402
from plan_amd import hip, loader  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parents[1]
OK, EINVAL, EUNSUPPORTED, EOVERFLOW = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_EOVERFLOW
DELTA, SNAPPY = hip.PH_PARQUET_DELTA, hip.PH_PARQUET_SNAPPY


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("delta_cases")


@pytest.fixture(scope="module")
def cases(files):
    return D.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column)


def test_the_flag_and_the_limits_are_the_headers():
    assert DELTA == 4 and DELTA | SNAPPY == 5
    text = (ROOT / "include" / "planhip.h").read_text()
    assert "#define PH_PARQUET_DELTA 4u" in text
    text = (ROOT / "plan_amd" / "csrc" / "parquet_decode.h").read_text()
    assert "DELTA_MAX_BLOCK = %d;" % D.MAX_BLOCK in text and "DELTA_MAX_MINIBLOCKS = %d;" % D.MAX_MINIBLOCKS in text


# ---------------------------------------------------------------- raw streams

@pytest.mark.parametrize("case", D.valid_streams(), ids=lambda c: c[0])
def test_crafted_streams_decode_as_the_format_says(case):
    name, stream, bits = case
    want, used, _widths = D.decode(stream, bits, exact=True)
    got, consumed = hip.delta_decode_host(stream, bits, exact=True)
    assert got.tolist() == want and consumed == used == len(stream)
    got, consumed = hip.delta_decode_host(stream + b"\xee\xee", bits, expected=len(want))     # bytes behind it are not its business
    assert got.tolist() == want and consumed == len(stream)


def test_crafted_streams_hold_what_they_are_meant_to():
    by = {name: (stream, bits) for name, stream, bits in D.valid_streams()}
    assert D.decode(*by["width_64_random"])[2] == {64} and D.decode(*by["width_32_random_int32"])[2] == {32}
    s, _b = by["first_value_and_min_delta_of_10_bytes"]
    assert s[4:14] == bytes([0xff] * 9 + [1]) and s[14:24] == bytes([0xff] * 9 + [1])          # zigzag(INT64_MIN) = 2^64 - 1, twice
    s, _b = by["junk_width_bytes_on_unneeded_miniblocks"]
    assert s.count(0xff) == 3                                                                  # 129 deltas: a block, and one miniblock of four
    vals, _u, _w = D.decode(*by["int32_stream_wraps_through_64_bit_sums"])
    assert vals == [D.I32_MAX, D.I32_MIN, D.I32_MIN + 1]
    assert hip.delta_decode_host(by["int32_stream_wraps_through_64_bit_sums"][0], 64)[0].tolist() == [D.I32_MAX, D.I32_MAX + 1, D.I32_MAX + 2]


@pytest.mark.parametrize("case", D.invalid_streams(), ids=lambda c: c[0])
def test_refused_streams(case):
    name, stream, bits, expected, word, unsupported = case
    with pytest.raises(D.Refused) as r:
        D.decode(stream, bits, expected, exact=True)
    assert r.value.unsupported == unsupported
    with pytest.raises(hip.PlanHipError) as e:
        hip.delta_decode_host(stream, bits, -1 if expected is None else expected, exact=True)
    assert e.value.code == (EUNSUPPORTED if unsupported else EINVAL) and word in str(e.value), str(e.value)


def test_a_count_above_the_room_is_capacity_before_anything_loops():
    s = hip.DeltaStream(0, 5, 64, 0, -1, 0, 0, 0, 0, 0, 0)
    stream = D.header(128, 4, 1 << 31, 0)
    s.src_bytes = len(stream)
    assert hip.lib().ph_delta_decode_host(stream, None, hip.ctypes.byref(s)) == hip.PH_ECAPACITY and s.count == 1 << 31
    with pytest.raises(hip.PlanHipError) as e:                     # a count no page can hold
        hip.delta_decode_host(D.header(128, 4, (1 << 31) + 1, 0), 64)
    assert e.value.code == EINVAL and "count" in str(e.value)


# ---------------------------------------------------------------- files

def read_and_compare(c, flags, types=None):
    data = c.data
    want_table = pq.read_table(c.path)
    for k, cname in enumerate(want_table.column_names):
        vals, valid, strs = C.expected_column(want_table.column(cname))
        got_vals, got_valid, off, byts = hip.parquet_read_column_host(data, k, flags=flags)
        assert np.array_equal(got_valid, valid), cname
        if strs is None:
            assert off is None and np.array_equal(got_vals, vals), cname
        else:
            assert got_vals is None and off[0] == 0 and off[-1] == len(byts) == sum(len(s) for s in strs), cname
            assert [byts[off[i]:off[i + 1]] for i in range(len(strs))] == strs, cname
    return data, want_table


@pytest.mark.parametrize("name", D.CASE_NAMES)
def test_host_twin_equals_read_table(cases, name):
    if name not in cases:
        pytest.skip("this pyarrow has no Snappy codec to write the file with")
    c, more = cases[name]
    data, table = read_and_compare(c, DELTA | more)
    if table.num_rows:                                             # without the flag: refused as before, naming the encoding
        k = [i for i, f in enumerate(table.schema) if not f.name.startswith("s40") or "dictionary" not in name][0]
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, k, flags=more)
        assert e.value.code == EUNSUPPORTED and "DELTA_" in str(e.value) and "PLAIN and RLE_DICTIONARY only" in str(e.value)


def test_writer_knobs_gave_the_pages_the_list_promises(cases):
    """every count in a page of its own, both page versions, many pages a chunk, three row groups, and every miniblock width of the list"""
    for n in D.COUNTS:
        for kind in ("nullable", "required") if n else ("nullable",):
            c, _m = cases["count_%d_%s" % (n, kind)]
            data = c.data
            for k in range(3):
                (p,) = pages_of(data, k)
                assert p["encoding"] == (D.E_DELTA_LENGTH_BYTE_ARRAY if k == 2 else D.E_DELTA_BINARY_PACKED)
                assert c.table.column(k).null_count == c.table.num_rows - n
    kinds = {name: {p["kind"] for p in pages_of(cases[name][0].data, 0)} for name in ("matrix_v1", "matrix_v2", "matrix_pages37_v1", "matrix_pages37_v2")}
    assert kinds == {"matrix_v1": {0}, "matrix_v2": {3}, "matrix_pages37_v1": {0}, "matrix_pages37_v2": {3}}
    assert len(pages_of(cases["matrix_pages37_v1"][0].data, 0)) == -(-D.MATRIX_ROWS // 37)
    assert {p["row_group"] for p in pages_of(cases["matrix_3groups"][0].data, 3)} == {0, 1, 2}
    c, _m = cases["widths_v1"]
    data = c.data
    seen = {}
    for k, f in enumerate(c.table.schema):
        if f.name.endswith("_n"):
            continue
        (p,) = pages_of(data, k)
        vals, used, widths = D.decode(data[p["data_pos"]:p["data_pos"] + p["data_bytes"]], 32 if f.type == pa.int32() else 64, p["num_values"], exact=True)
        assert vals == c.table.column(k).to_pylist() and used == p["data_bytes"], f.name   # the stream ends exactly at the page's end
        seen[f.name] = widths
    assert seen["stride"] == {0} and seen["steps01"] == {1} and seen["w64"] == {64} and seen["w32_i32"] == {32}
    assert max(seen["alt64"]) <= 2 and max(seen["alt32"]) <= 2       # (MAX - MIN wraps to -1: the extremes are one step apart)
    for w in (7, 8, 9, 31, 32, 33, 63):
        assert seen["w%d" % w] == {w}
    assert len(seen["mixed_widths"]) > 1 and min(seen["mixed_widths"]) <= 2 and max(seen["mixed_widths"]) >= 48
    # a dictionary column beside delta columns of one file
    c, _m = cases["dictionary_beside_delta"]
    encs = [{p["encoding"] for p in pages_of(c.data, k) if p["kind"] != 2} for k in range(c.table.num_columns)]
    assert {8} in encs and {5} in encs and {6} in encs


def test_type_mappings_and_overrides(cases):
    c, _m = cases["overrides"]
    data = c.data
    names = c.table.column_names
    small = np.asarray(c.table.column("small64").to_numpy())
    i32 = c.table.column("i32").to_numpy().astype(np.int64)
    for typ, scale, col, want in ((hip.PH_I64, 0, "i32", i32), (hip.PH_I32, 0, "small64", small), (hip.PH_DEC64, 2, "small64", small), (hip.PH_DEC64, 4, "i32", i32)):
        got, valid, _o, _b = hip.parquet_read_column_host(data, names.index(col), typ, scale, flags=DELTA)
        assert np.array_equal(got, want) and valid.all(), (typ, col)
    vals, valid, _s = C.expected_column(c.table.column("small64_n"))
    got, gvalid, _o, _b = hip.parquet_read_column_host(data, names.index("small64_n"), hip.PH_I32, 0, flags=DELTA)
    assert np.array_equal(got, vals) and np.array_equal(gvalid, valid)
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(data, names.index("big64"), hip.PH_I32, 0, flags=DELTA)
    assert e.value.code == EOVERFLOW and "int32" in str(e.value) and "(big64)" in str(e.value) and "page 0" in str(e.value)
    assert np.array_equal(hip.parquet_read_column_host(data, names.index("big64"), flags=DELTA)[0], c.table.column("big64").to_numpy())
    # the schema's own mappings: a date and the integer-stored decimals are delta pages in the matrix
    c, _m = cases["matrix_v1"]
    info = {col["name"]: col for col in loader.parquet_schema(c.path)["columns"]}
    assert (info["date_r"]["type"], info["d9_r"]["type"], info["d9_r"]["physical_type"], info["d15_n"]["physical_type"], info["d15_n"]["scale"]) == (hip.PH_DATE, hip.PH_DEC64, 1, 2, 2)
    assert {p["encoding"] for k in range(c.table.num_columns) for p in pages_of(c.data, k)} == {5, 6}


def test_without_the_flag_nothing_changes(files):
    delta = C.refusals(files)["delta"][0]
    dl = D.delta_length_file(files)
    for path, enc in ((delta, "DELTA_BINARY_PACKED"), (dl, "DELTA_LENGTH_BYTE_ARRAY")):
        data = open(path, "rb").read()
        msgs = []
        for call in (lambda: hip.parquet_read_column_host(data, 0), lambda: hip.parquet_read_column_host(data, 0, flags=0)):
            with pytest.raises(hip.PlanHipError) as e:
                call()
            assert e.value.code == EUNSUPPORTED
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1] == "planhip error -3: ph_parquet_read_column_host: column 0 (%s): row group 0, page 0: %s values; PLAIN and RLE_DICTIONARY only" % (
            "i" if enc == "DELTA_BINARY_PACKED" else "s", enc)
        hip.parquet_read_column_host(data, 0, flags=DELTA)          # and with it they read
    assert np.array_equal(hip.parquet_read_column_host(open(delta, "rb").read(), 1)[0], np.arange(100))


def test_other_encodings_stay_unsupported_with_the_flag(files):
    for name, (path, col, enc) in D.unsupported_files(files).items():
        data = open(path, "rb").read()
        names = pq.read_table(path).column_names
        for flags in (DELTA, DELTA | SNAPPY):
            with pytest.raises(hip.PlanHipError) as e:
                hip.parquet_read_column_host(data, names.index(col), flags=flags)
            assert e.value.code == EUNSUPPORTED and (enc + " values") in str(e.value) and "(%s)" % col in str(e.value), str(e.value)
        hip.parquet_read_column_host(data, 1 - names.index(col), flags=DELTA)           # only the requested column is judged


def test_flag_values(cases):
    data = cases["count_33_required"][0].data
    for flags in (2, 3, 6, 7, 8, 0x80000000):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, 0, flags=flags)
        assert e.value.code == EINVAL and "flags" in str(e.value) and "PH_PARQUET_SNAPPY" in str(e.value) and "PH_PARQUET_DELTA" in str(e.value)
    # a PLAIN file reads the same with the flag
    plain = D.plain_twin(pathlib.Path(cases["count_33_required"][0].path).parent, "count_33_flag", cases["count_33_required"][0].table)
    for k in range(3):
        a, b = hip.parquet_read_column_host(plain.data, k), hip.parquet_read_column_host(plain.data, k, flags=DELTA)
        assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def test_one_byte_patches(files):
    what = {"header_count": "fewer or more values", "width_65": "malformed DELTA_BINARY_PACKED", "block_size": "malformed DELTA_BINARY_PACKED",
            "length_negative": "BYTE_ARRAY length", "lengths_sum_past": "BYTE_ARRAY length", "lengths_sum_short": "fewer or more values"}
    for name, (orig, bad, column, page) in D.patched(files, pages_of).items():
        good = hip.parquet_read_column_host(orig, column, flags=DELTA)
        assert good[0] is not None or good[3]
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(bad, column, flags=DELTA)
        msg = str(e.value)
        assert e.value.code == EINVAL and ("column %d (" % column) in msg and ("row group 0, page %d:" % page) in msg, (name, msg)
        (word,) = [w for k, w in what.items() if k in name]
        assert word in msg, (name, msg)
        # what pyarrow does with it: a tolerated_ file is read (this build still refuses it), every other one raises
        try:
            pq.read_table(pa.BufferReader(bad))
            read = True
        except Exception:  # noqa: BLE001
            read = False
        assert read == name.startswith("tolerated_"), name
    both, column = D.two_bad_pages(files, pages_of)
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(both, column, flags=DELTA)
    assert e.value.code == EINVAL and "page 1:" in str(e.value)


# ---------------------------------------------------------------- the sanitizer

SANITIZER_PROGRAM = r"""
#include "parquet_decode.h"
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

// argv: files. *.stream = [bits: 1 byte][exact: 1 byte][expected count: 8 bytes, little-endian, -1 = any][ONE raw DELTA_BINARY_PACKED stream],
// decoded from a buffer of exactly the stream's length into a buffer of exactly the header's count. Everything else = a Parquet file: every
// leaf column resolved and decoded with PH_PARQUET_SNAPPY | PH_PARQUET_DELTA by the functions the kernels instantiate. A refused input is
// fine (it is counted), a read or write out of range is the sanitizer's to report.
static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream in(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    return std::vector<uint8_t>(raw.begin(), raw.end());
}

int main(int argc, char **argv) {
    long decoded = 0, refused = 0;
    for (int a = 1; a < argc; a++) {
        const std::string path = argv[a];
        std::vector<uint8_t> file = slurp(argv[a]);                 // exactly nbytes: one byte past the end is out of range
        if (path.size() > 7 && path.compare(path.size() - 7, 7, ".stream") == 0) {
            const int bits = file[0], exact = file[1];
            int64_t expected = 0;
            memcpy(&expected, file.data() + 2, 8);
            std::vector<uint8_t> stream(file.begin() + 10, file.end());
            const ph::pq::HostBytes g(stream.data());
            int64_t pos = 0, count = 0;
            int cause = 0;
            int sub = ph::pq::host_delta_stream(g, pos, (int64_t)stream.size(), bits, expected, 0, &count, &cause, [](int64_t, int64_t) { return 0; });
            if (sub == ph::pq::DS_CAPACITY && count <= (1 << 20)) {
                std::vector<int64_t> out((size_t)count);
                pos = 0;
                sub = ph::pq::host_delta_stream(g, pos, (int64_t)stream.size(), bits, expected, count, &count, &cause, [&](int64_t k, int64_t v) { out[(size_t)k] = v; return 0; });
            }
            if (sub == ph::pq::DS_OK && exact && pos != (int64_t)stream.size()) sub = ph::pq::DS_TRAILING;
            if (sub != ph::pq::DS_OK) refused++;
            else decoded++;
            continue;
        }
        ph::pq::FileMeta fm;
        ph::pq::Status st;
        if (ph::pq::parse_footer(file.data(), (int64_t)file.size(), &fm, &st) != PH_OK) { refused++; continue; }
        for (size_t c = 0; c < fm.leaves.size(); c++) {
            ph::pq::ColPlan cp;
            ph::pq::Status s2;
            if (ph::pq::resolve_column(file.data(), (int64_t)file.size(), fm, (int32_t)c, 0, 0, &cp, &s2, PH_PARQUET_SNAPPY | PH_PARQUET_DELTA) != PH_OK || fm.num_rows >= (1ll << 31)) { refused++; continue; }
            std::vector<int64_t> values((size_t)fm.num_rows + 1);
            std::vector<uint8_t> valid((size_t)fm.num_rows + 1);
            std::vector<int32_t> off((size_t)fm.num_rows + 1);
            int64_t total = 0;
            if (ph::pq::decode_column_host(file.data(), cp, fm.num_rows, values.data(), valid.data(), off.data(), nullptr, 0, &total, &s2) != PH_OK) { refused++; continue; }
            std::vector<char> bytes((size_t)total + 1);
            if (ph::pq::decode_column_host(file.data(), cp, fm.num_rows, values.data(), valid.data(), off.data(), bytes.data(), total, &total, &s2) != PH_OK) { refused++; continue; }
            decoded++;
        }
    }
    std::printf("decoded %ld refused %ld\n", decoded, refused);
    return 0;
}
"""


def test_decoders_under_address_sanitizer(cases, files, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the sanitizer check of the delta decoders needs a C++17 host compiler")
    src = tmp_path / "delta_asan.cpp"
    src.write_text(SANITIZER_PROGRAM)
    exe = tmp_path / "delta_asan"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         f"-I{ROOT / 'plan_amd' / 'csrc'}", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    paths = []
    valid, invalid = D.valid_streams(), D.invalid_streams()
    streams = [(name, stream, bits, None) for name, stream, bits in valid] + [(name, stream, bits, expected) for name, stream, bits, expected, _w, _u in invalid]
    for name, stream, bits, expected in streams:
        p = tmp_path / (name + ".stream")
        p.write_bytes(bytes([bits, 1]) + int(-1 if expected is None else expected).to_bytes(8, "little", signed=True) + stream)
        paths.append(str(p))
    file_paths, good, bad = D.write_all(files, pages_of)
    run = subprocess.run([str(exe)] + paths + file_paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    decoded, refused = (int(x) for x in run.stdout.split()[1::2])
    assert decoded == len(valid) + good and refused == len(invalid) + bad, run.stdout
