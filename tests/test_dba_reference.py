"""Front-coded pages of the Parquet load path (DELTA_BYTE_ARRAY, PH_PARQUET_DELTA_BYTE_ARRAY), without a GPU. The raw host decoder
(ph_delta_byte_array_decode_host, the host twin the kernels are written against) against the spec-restating decoder of tests/dba_cases.py on
crafted sections, valid and refused, and that decoder against the values sections pyarrow writes; ph_parquet_read_column_host_ex with the
flag against pq.read_table value by value on pyarrow-written files (counts at the lane, workgroup and block edges, the string shapes, v1 /
v2 pages, 37 rows a page, three row groups, every codec, a dictionary and a DELTA_LENGTH_BYTE_ARRAY column beside the front-coded ones); the
flag matrix and the refusals with and without the flag; one-byte patches; and all of it once more in a stand-alone program under
AddressSanitizer. Bytes and integers: equality is the tolerance."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

import dba_cases as B  # noqa: E402
import delta_cases as D  # noqa: E402
import parquet_cases as C  # noqa: E402
from plan_amd import hip, loader  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parents[1]
OK, EINVAL, EUNSUPPORTED, ECAPACITY = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_ECAPACITY
DBA, DELTA, SNAPPY = hip.PH_PARQUET_DELTA_BYTE_ARRAY, hip.PH_PARQUET_DELTA, hip.PH_PARQUET_SNAPPY
CODES = {"EINVAL": EINVAL, "EUNSUPPORTED": EUNSUPPORTED}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("dba_cases")


@pytest.fixture(scope="module")
def cases(files):
    return B.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column)


def test_the_flag_and_the_ring_are_the_headers():
    assert DBA == 1024 and DBA & (DBA - 1) == 0
    assert "#define PH_PARQUET_DELTA_BYTE_ARRAY 1024u" in (ROOT / "include" / "planhip.h").read_text()
    assert "DBA_RING = %d;" % B.RING in (ROOT / "plan_amd" / "csrc" / "dba_decode.h").read_text()


# ---------------------------------------------------------------- raw sections

@pytest.mark.parametrize("case", B.valid_sections(), ids=lambda c: c[0])
def test_crafted_sections_decode_as_the_format_says(case):
    name, data, values = case
    assert B.decode(data) == values
    lens, byts, s = hip.delta_byte_array_decode_host(data)
    assert lens.tolist() == [len(v) for v in values] and byts == b"".join(values)
    assert (s.count, s.total_bytes, s.consumed, s.status, s.sub) == (len(values), len(byts), len(data), OK, 0)
    lens, byts, s = hip.delta_byte_array_decode_host(data, expected=len(values))
    assert byts == b"".join(values)


@pytest.mark.parametrize("case", B.invalid_sections(), ids=lambda c: c[0])
def test_refused_sections(case):
    name, data, expected, word, code = case
    with pytest.raises(B.Refused) as r:
        B.decode(data, expected)
    assert r.value.unsupported == (code == "EUNSUPPORTED")
    with pytest.raises(hip.PlanHipError) as e:
        hip.delta_byte_array_decode_host(data, -1 if expected is None else expected)
    assert e.value.code == CODES[code] and word in str(e.value), str(e.value)
    assert e.value.record.consumed == 0


def test_the_rooms_are_capacity_and_nothing_outside_them_is_written():
    name, data, values = [c for c in B.valid_sections() if c[0] == "sorted_keys"][0]
    total = sum(len(v) for v in values)
    for lroom, broom, count, reported in ((len(values) - 1, total, len(values), 0), (len(values), total - 1, len(values), total), (0, 0, len(values), 0)):
        s = hip.DbaStream(0, len(data), -1, 2, lroom, 3, broom, 0, 0, 0, 0, 0)
        lens, byts = np.full(lroom + 4, -7, np.int32), np.full(broom + 6, 0x5a, np.uint8)
        rc = hip.lib().ph_delta_byte_array_decode_host(data, hip.vp(lens.ctypes.data), hip.vp(byts.ctypes.data), hip.ctypes.byref(s))
        assert (rc, s.status, s.count, s.total_bytes, s.consumed) == (ECAPACITY, ECAPACITY, count, reported, 0)
        assert (lens == -7).all() and (byts == 0x5a).all()
    s = hip.DbaStream(0, len(data), -1, 2, len(values), 3, total, 0, 0, 0, 0, 0)
    lens, byts = np.full(len(values) + 4, -7, np.int32), np.full(total + 6, 0x5a, np.uint8)
    assert hip.lib().ph_delta_byte_array_decode_host(data, hip.vp(lens.ctypes.data), hip.vp(byts.ctypes.data), hip.ctypes.byref(s)) == OK
    assert lens[:2].tolist() == [-7, -7] and lens[-2:].tolist() == [-7, -7] and lens[2:-2].tolist() == [len(v) for v in values]
    assert byts[3:-3].tobytes() == b"".join(values) and (byts[:3] == 0x5a).all() and (byts[-3:] == 0x5a).all()


def test_the_expansion_bomb_is_refused_from_its_lengths_alone():
    data = B.bomb()
    assert len(data) - 70000 < 6000                 # both streams in under 6 KB, and one suffix byte a value
    n = 70000
    s = hip.DbaStream(0, len(data), -1, 0, n, 0, 1 << 20, 0, 0, 0, 0, 0)
    lens, byts = np.full(n, -7, np.int32), np.full(1 << 20, 0x5a, np.uint8)
    rc = hip.lib().ph_delta_byte_array_decode_host(data, hip.vp(lens.ctypes.data), hip.vp(byts.ctypes.data), hip.ctypes.byref(s))
    assert (rc, s.count, s.total_bytes) == (EINVAL, n, n * (n + 1) // 2) and s.total_bytes >= 1 << 31
    assert (lens == -7).all() and (byts == 0x5a).all()
    # one value fewer than 2^31 bytes need: the room decides, and still nothing is written
    m = 65535                                       # 65535 * 65536 / 2 = 2^31 - 32768
    small = B.section(list(range(m)), [1] * m, b"z" * m)
    s = hip.DbaStream(0, len(small), -1, 0, n, 0, 1 << 20, 0, 0, 0, 0, 0)
    rc = hip.lib().ph_delta_byte_array_decode_host(small, hip.vp(lens.ctypes.data), hip.vp(byts.ctypes.data), hip.ctypes.byref(s))
    assert (rc, s.count, s.total_bytes) == (ECAPACITY, m, (1 << 31) - 32768) and (lens == -7).all() and (byts == 0x5a).all()


def test_the_restated_decoder_reads_what_pyarrow_writes(cases):
    """the values sections of pyarrow-written required columns, one page each, through the Python decoder: the restatement is pinned"""
    seen = 0
    for name in ("count_513_required", "count_129_required", "shape_prefix_257", "shape_ring_%d" % (B.RING + 1), "shape_identical", "shape_nothing_shared"):
        c, _f = cases[name]
        data = c.data
        for k, f in enumerate(c.table.schema):
            if c.table.column(k).null_count:
                continue
            (p,) = pages_of(data, k)
            assert p["encoding"] == B.E_DELTA_BYTE_ARRAY and p["kind"] == 0
            want = [v if isinstance(v, bytes) else v.encode() for v in c.table.column(k).to_pylist()]
            at = p["data_pos"]
            if f.nullable:                                          # a v1 page: [4-byte length][definition levels] in front of the values
                at += 4 + int.from_bytes(data[at:at + 4], "little")
            assert B.decode(data[at:p["data_pos"] + p["data_bytes"]], p["num_values"]) == want, (name, f.name)
            seen += 1
    assert seen >= 6


# ---------------------------------------------------------------- files

def read_and_compare(c, flags):
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


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_host_twin_equals_read_table(cases, name):
    if name not in cases:
        pytest.skip("this pyarrow has no codec to write the file with")
    c, more = cases[name]
    data, table = read_and_compare(c, DBA | more)
    if table.num_rows:                                             # without the flag: refused as before, naming the encoding
        k = [i for i, f in enumerate(table.schema) if {p["encoding"] for p in loader.parquet_pages(data, i, codecs=True) if p["kind"] != 2} == {B.E_DELTA_BYTE_ARRAY}][0]
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, k, flags=more)
        assert e.value.code == EUNSUPPORTED and "DELTA_BYTE_ARRAY values" in str(e.value)


def test_writer_knobs_gave_the_pages_the_list_promises(cases):
    for n in B.COUNTS:
        for kind in ("nullable", "required") if n else ("nullable",):
            c, _m = cases["count_%d_%s" % (n, kind)]
            for k in range(2):
                (p,) = pages_of(c.data, k)
                assert p["encoding"] == B.E_DELTA_BYTE_ARRAY and c.table.column(k).null_count == c.table.num_rows - n
    kinds = {name: {p["kind"] for p in pages_of(cases[name][0].data, 0)} for name in ("matrix_v1", "matrix_v2", "matrix_pages37_v1", "matrix_pages37_v2")}
    assert kinds == {"matrix_v1": {0}, "matrix_v2": {3}, "matrix_pages37_v1": {0}, "matrix_pages37_v2": {3}}
    assert len(pages_of(cases["matrix_pages37_v1"][0].data, 0)) == -(-B.MATRIX_ROWS // 37)
    assert {p["row_group"] for p in pages_of(cases["matrix_3groups"][0].data, 3)} == {0, 1, 2}
    c, more = cases["beside_dictionary_and_delta_length"]
    assert more == DELTA
    encs = {f.name: {p["encoding"] for p in pages_of(c.data, k) if p["kind"] != 2} for k, f in enumerate(c.table.schema)}
    assert encs["s40_r"] == {8} and encs["text_n"] == {6} and encs["sorted_r"] == {7} and encs["none_r"] == {0} and encs["i64"] == {5}
    # front coding does what it is for: sorted keys take a fraction of their PLAIN bytes
    c, _m = cases["matrix_v1"]
    k = c.table.column_names.index("sorted_r")
    assert pages_of(c.data, k)[0]["data_bytes"] * 3 < sum(len(v) + 4 for v in c.table.column(k).to_pylist())


def test_flag_matrix(cases, files):
    c, _m = cases["count_33_required"]
    data = c.data
    plain = B.plain_twin(files, "count_33_flag", c.table)
    for k in range(2):                                             # 1024 alone reads an uncompressed PLAIN file as flags 0 does
        a, b = hip.parquet_read_column_host(plain.data, k), hip.parquet_read_column_host(plain.data, k, flags=DBA)
        assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
    msgs = []
    for flags in (None, 0, DELTA, DELTA | SNAPPY):                 # without it the refusal is what it was
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, 0) if flags is None else hip.parquet_read_column_host(data, 0, flags=flags)
        assert e.value.code == EUNSUPPORTED
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] == "planhip error -3: ph_parquet_read_column_host: column 0 (sorted): row group 0, page 0: DELTA_BYTE_ARRAY values; PLAIN and RLE_DICTIONARY only"
    assert msgs[2] == msgs[3] == ("planhip error -3: ph_parquet_read_column_host: column 0 (sorted): row group 0, page 0: DELTA_BYTE_ARRAY values of a BYTE_ARRAY column; "
                                  "PLAIN, RLE_DICTIONARY, DELTA_BINARY_PACKED (INT32 / INT64) and DELTA_LENGTH_BYTE_ARRAY (BYTE_ARRAY) only")
    for flags in (2048, 1024 | 2, 512, 1024 | 512, 0x80000000 | 1024):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, 0, flags=flags)
        msg = str(e.value)
        assert e.value.code == EINVAL and "flags" in msg and msg.endswith("and PH_PARQUET_ZSTD are defined"), msg
        assert all(n in msg for n in ("PH_PARQUET_SNAPPY", "PH_PARQUET_DELTA,", "PH_PARQUET_DELTA_BYTE_ARRAY", "PH_PARQUET_LZ4_RAW", "PH_PARQUET_GZIP"))
    # the flag does not enable the other delta encodings
    dl = D.delta_length_file(files)
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(open(dl, "rb").read(), 0, flags=DBA)
    assert e.value.code == EUNSUPPORTED and "DELTA_LENGTH_BYTE_ARRAY values; PLAIN and RLE_DICTIONARY only" in str(e.value)
    hip.parquet_read_column_host(open(dl, "rb").read(), 0, flags=DBA | DELTA)


def test_other_uses_stay_unsupported_with_the_flag(files):
    for name, (path, col, enc, phys) in B.unsupported_files(files).items():
        data = open(path, "rb").read()
        names = pq.read_table(path).column_names
        for flags in (DBA, DBA | DELTA, DBA | DELTA | SNAPPY):
            with pytest.raises(hip.PlanHipError) as e:
                hip.parquet_read_column_host(data, names.index(col), flags=flags)
            msg = str(e.value)
            assert e.value.code == EUNSUPPORTED and (enc + " values") in msg and "(%s)" % col in msg and (phys is None or phys in msg), msg
        hip.parquet_read_column_host(data, names.index("s"), flags=DBA)                # only the requested column is judged


def test_one_byte_patches(files):
    for name, (orig, bad, column, page, word) in B.patched(files, pages_of).items():
        good = hip.parquet_read_column_host(orig, column, flags=DBA)
        assert good[3] == "".join(B.PATCH_VALUES).encode()
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(bad, column, flags=DBA)
        msg = str(e.value)
        assert e.value.code == EINVAL and ("column %d (" % column) in msg and ("row group 0, page %d:" % page) in msg and word in msg, (name, msg)
        # what pyarrow does with it: a tolerated_ file is read (this build still refuses it), every other one raises
        try:
            pq.read_table(pa.BufferReader(bad))
            read = True
        except Exception:  # noqa: BLE001
            read = False
        assert read == name.startswith("tolerated_"), name
    both, column = B.two_bad_pages(files, pages_of)
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(both, column, flags=DBA)
    assert e.value.code == EINVAL and "page 1:" in str(e.value) and "fewer or more values" in str(e.value)
    mixed = B.front_and_compressed(files, lambda d, k: loader.parquet_pages(d, k, codecs=True))
    if mixed is not None:
        data, s_page, z_page = mixed
        for column, page, word in ((0, s_page, "fewer or more values"), (1, z_page, "corrupt SNAPPY")):
            with pytest.raises(hip.PlanHipError) as e:
                hip.parquet_read_column_host(data, column, flags=DBA | SNAPPY)
            assert e.value.code == EINVAL and ("page %d:" % page) in str(e.value) and word in str(e.value), str(e.value)


# ---------------------------------------------------------------- the sanitizer

SANITIZER_PROGRAM = r"""
#include "parquet_decode.h"
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

// argv: files. *.section = [expected count: 8 bytes, little-endian, -1 = any][ONE raw DELTA_BYTE_ARRAY values section], decoded by
// ph_delta_byte_array_decode_host's function from a buffer of exactly the section's length: first with no room at all, then with exactly the
// room the first call reports. Everything else = a Parquet file: every leaf column resolved and decoded with every flag set by the functions
// the kernels are written against. A refused input is fine (it is counted), a read or write out of range is the sanitizer's to report.
static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream in(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    return std::vector<uint8_t>(raw.begin(), raw.end());
}

int main(int argc, char **argv) {
    long decoded = 0, refused = 0;
    const uint32_t flags = PH_PARQUET_SNAPPY | PH_PARQUET_DELTA | PH_PARQUET_LZ4_RAW | PH_PARQUET_GZIP | PH_PARQUET_ZSTD | PH_PARQUET_DELTA_BYTE_ARRAY;
    for (int a = 1; a < argc; a++) {
        const std::string path = argv[a];
        std::vector<uint8_t> file = slurp(argv[a]);                 // exactly nbytes: one byte past the end is out of range
        if (path.size() > 8 && path.compare(path.size() - 8, 8, ".section") == 0) {
            int64_t expected = 0;
            memcpy(&expected, file.data(), 8);
            std::vector<uint8_t> sec(file.begin() + 8, file.end());
            ph_dba_stream s{};
            s.src_bytes = (int64_t)sec.size();
            s.expected = expected;
            int sub = ph::pq::host_dba_section(sec.data(), &s, nullptr, nullptr);
            if (s.status == PH_ECAPACITY && s.count <= (1 << 20)) {
                std::vector<int32_t> lens((size_t)s.count);
                s.len_cap = s.count;
                sub = ph::pq::host_dba_section(sec.data(), &s, lens.data(), nullptr);
                if (s.status == PH_ECAPACITY && s.total_bytes <= (1 << 26)) {
                    std::vector<char> bytes((size_t)s.total_bytes);
                    s.byte_cap = s.total_bytes;
                    sub = ph::pq::host_dba_section(sec.data(), &s, lens.data(), bytes.data());
                }
            }
            if (sub != ph::pq::DBA_OK) refused++;
            else decoded++;
            continue;
        }
        ph::pq::FileMeta fm;
        ph::pq::Status st;
        if (ph::pq::parse_footer(file.data(), (int64_t)file.size(), &fm, &st) != PH_OK) { refused++; continue; }
        for (size_t c = 0; c < fm.leaves.size(); c++) {
            ph::pq::ColPlan cp;
            ph::pq::Status s2;
            if (ph::pq::resolve_column(file.data(), (int64_t)file.size(), fm, (int32_t)c, 0, 0, &cp, &s2, flags) != PH_OK || fm.num_rows >= (1ll << 31)) { refused++; continue; }
            std::vector<int64_t> values((size_t)fm.num_rows + 1);
            std::vector<uint8_t> valid((size_t)fm.num_rows + 1);
            std::vector<int32_t> off((size_t)fm.num_rows + 1);
            int64_t total = 0;
            if (ph::pq::decode_column_host(file.data(), cp, fm.num_rows, values.data(), valid.data(), off.data(), nullptr, 0, &total, &s2) != PH_OK) { refused++; continue; }
            std::vector<char> bytes((size_t)total);                 // exactly the column's bytes
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
        pytest.fail("g++ not found: the sanitizer check of the front-coding decoders needs a C++17 host compiler")
    src = tmp_path / "dba_asan.cpp"
    src.write_text(SANITIZER_PROGRAM)
    exe = tmp_path / "dba_asan"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         f"-I{ROOT / 'plan_amd' / 'csrc'}", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    paths = []
    valid, invalid = B.valid_sections(), B.invalid_sections()
    sections = [(name, data, None) for name, data, _v in valid] + [(name, data, expected) for name, data, expected, _w, _c in invalid]
    for name, data, expected in sections:
        p = tmp_path / (name + ".section")
        p.write_bytes(int(-1 if expected is None else expected).to_bytes(8, "little", signed=True) + data)
        paths.append(str(p))
    file_paths, good, bad = B.write_all(files, pages_of)
    mixed = B.front_and_compressed(files, lambda d, k: loader.parquet_pages(d, k, codecs=True))
    if mixed is not None:
        p = tmp_path / "bad_front_and_compressed.parquet"
        p.write_bytes(mixed[0])
        file_paths.append(str(p))
        bad += 2
    run = subprocess.run([str(exe)] + paths + file_paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    decoded, refused = (int(x) for x in run.stdout.split()[1::2])
    assert decoded == len(valid) + good and refused == len(invalid) + bad, run.stdout
