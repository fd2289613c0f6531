"""The Parquet load path's host side, without a GPU: ph_parquet_schema and ph_parquet_pages against pyarrow's metadata, and
ph_parquet_read_column_host — the slow twin that runs the kernels' own __host__ __device__ decoders — against pq.read_table, value by
value. Integers and bytes: equality is the tolerance. Then everything that must be refused: outside the subset (PH_EUNSUPPORTED), bad
overrides, files the host checks reject, and one-byte patches that only decoding can see (PH_EINVAL, never a read out of range: a
stand-alone program under AddressSanitizer decodes every file of this module)."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

import parquet_cases as C  # noqa: E402
from plan_amd import hip, loader  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parents[1]
OK, EINVAL, EUNSUPPORTED, EOVERFLOW = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_EOVERFLOW
PHYS = {"BOOLEAN": 0, "INT32": 1, "INT64": 2, "INT96": 3, "FLOAT": 4, "DOUBLE": 5, "BYTE_ARRAY": 6, "FIXED_LEN_BYTE_ARRAY": 7}
ENC = {"PLAIN": 0, "PLAIN_DICTIONARY": 2, "RLE": 3, "BIT_PACKED": 4, "RLE_DICTIONARY": 8}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("parquet_cases")


@pytest.fixture(scope="module")
def cases(files):
    return C.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column)


def mapped_type(t):
    if pa.types.is_int32(t):
        return hip.PH_I32, 0
    if pa.types.is_int64(t):
        return hip.PH_I64, 0
    if pa.types.is_date32(t):
        return hip.PH_DATE, 0
    if pa.types.is_decimal(t):
        return hip.PH_DEC64, t.scale
    return hip.PH_STR, 0


CASE_NAMES = ["matrix_v1", "matrix_v2", "matrix_pages13", "matrix_pages37_v2", "matrix_pages37_v1_plain", "matrix_plain_v2", "matrix_decint_3groups",
              "matrix_3groups_pages37", "matrix_fallback", "matrix_fallback_v2_3groups", "matrix_dict_some"] + \
             ["rows_%d" % n for n in (0, 1, 7, 8, 9, 63, 64, 65, C.ROW_PAD - 1, C.ROW_PAD + 1)] + \
             ["nulls_v1", "nulls_v2_plain", "dict_widths", "dict_widths_pages37_v2", "dict_width17", "binary"] + \
             ["varchar_" + k + s for k in ("256_nulls", "256_empty_nulls", "257", "nul_byte", "empty", "long", "straddle") for s in ("", "_plain")]


def test_case_list_is_complete(cases):
    assert sorted(CASE_NAMES) == sorted(cases)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_schema_against_pyarrow_metadata(cases, name):
    c = cases[name]
    f = pq.ParquetFile(c.path)
    s = loader.parquet_schema(c.path)
    assert s["rows"] == f.metadata.num_rows == c.table.num_rows and s["row_groups"] == f.metadata.num_row_groups
    assert len(s["columns"]) == len(f.schema)
    for k, got in enumerate(s["columns"]):
        want = f.schema.column(k)
        field = c.table.schema.field(k)
        assert got["name"] == want.name == field.name
        assert got["physical_type"] == PHYS[want.physical_type], want.name
        assert (got["type"], got["scale"]) == mapped_type(field.type), want.name
        assert got["nullable"] == field.nullable == (want.max_definition_level == 1), want.name
        if want.physical_type == "FIXED_LEN_BYTE_ARRAY":
            assert got["type_length"] == want.length
    assert loader.parquet_schema(c.data) == s                     # bytes and a path are the same file


@pytest.mark.parametrize("name", CASE_NAMES)
def test_page_directory_against_pyarrow_metadata(cases, name):
    c = cases[name]
    md = pq.ParquetFile(c.path).metadata
    data = c.data
    for k in range(md.num_columns):
        pages = pages_of(data, k)
        row0 = 0
        for g in range(md.num_row_groups):
            cc = md.row_group(g).column(k)
            mine = [p for p in pages if p["row_group"] == g]
            if md.row_group(g).num_rows == 0 and not mine:
                continue
            first = cc.dictionary_page_offset if cc.has_dictionary_page and cc.dictionary_page_offset else cc.data_page_offset
            assert mine[0]["header_pos"] == first, (k, g)
            assert sum(p["data_pos"] - p["header_pos"] + p["data_bytes"] for p in mine) == cc.total_compressed_size, (k, g)
            datap = [p for p in mine if p["kind"] in (hip.PH_PARQUET_PAGE_DATA, hip.PH_PARQUET_PAGE_DATA_V2)]
            assert sum(p["num_values"] for p in datap) == cc.num_values == md.row_group(g).num_rows
            assert {p["encoding"] for p in mine} <= {ENC[e] for e in cc.encodings if e in ENC}, (k, g, cc.encodings)
            assert [p["kind"] for p in mine].count(hip.PH_PARQUET_PAGE_DICTIONARY) == (1 if cc.has_dictionary_page else 0)
            run = row0
            for p in datap:
                assert p["first_row"] == run
                run += p["num_values"]
            for a, b in zip(mine, mine[1:]):
                assert a["data_pos"] + a["data_bytes"] == b["header_pos"]
            row0 += md.row_group(g).num_rows
        assert row0 == md.num_rows


def test_writer_knobs_gave_the_awkward_pages(cases):
    """the cases hold what they are meant to: 13 / 26- and 37-row pages, both page versions, three row groups, a dictionary chunk that falls
    back to PLAIN, both decimal layouts, index widths up to 17 bits"""
    def sizes(name, col):
        return [p["num_values"] for p in pages_of(cases[name].data, col) if p["kind"] != hip.PH_PARQUET_PAGE_DICTIONARY]
    small = set().union(*[set(sizes("matrix_pages13", k)[:-1]) for k in range(14)])
    assert 13 in small and small <= {13, 26}, small            # (26 where two batches fit the 64 bytes)
    assert set(sizes("matrix_pages37_v2", 2)[:-1]) == {37}
    kinds = lambda name: {p["kind"] for p in pages_of(cases[name].data, 0)}  # noqa: E731
    assert hip.PH_PARQUET_PAGE_DATA in kinds("matrix_v1") and hip.PH_PARQUET_PAGE_DATA_V2 in kinds("matrix_v2")
    assert loader.parquet_schema(cases["matrix_decint_3groups"].path)["row_groups"] == 3
    names = cases["matrix_v1"].table.column_names
    fb = pages_of(cases["matrix_fallback"].data, names.index("i64_r"))
    encs = [p["encoding"] for p in fb if p["kind"] != hip.PH_PARQUET_PAGE_DICTIONARY]
    assert encs[0] in (2, 8) and encs[-1] == 0, encs          # RLE_DICTIONARY first, PLAIN after the dictionary outgrew its limit
    cols = {c["name"]: c for c in loader.parquet_schema(cases["matrix_v1"].path)["columns"]}
    assert (cols["d9_n"]["physical_type"], cols["d9_n"]["type_length"]) == (7, 4) and (cols["d15_n"]["physical_type"], cols["d15_n"]["type_length"]) == (7, 7)
    cols = {c["name"]: c for c in loader.parquet_schema(cases["matrix_decint_3groups"].path)["columns"]}
    assert cols["d9_r"]["physical_type"] == 1 and cols["d15_r"]["physical_type"] == 2
    # index widths: the byte in front of a dictionary-coded page's runs
    d = cases["dict_width17"].data
    def width(d, p):          # a nullable column's v1 page: [4-byte length][levels][bit width][runs]
        return d[p["data_pos"] + 4 + int.from_bytes(d[p["data_pos"]:p["data_pos"] + 4], "little")]
    coded = [p for p in pages_of(d, 0) if p["encoding"] in (2, 8) and p["kind"] == hip.PH_PARQUET_PAGE_DATA]
    assert max(width(d, p) for p in coded) == 17
    d = cases["dict_widths"].data
    widths = [width(d, [p for p in pages_of(d, k) if p["kind"] == hip.PH_PARQUET_PAGE_DATA][0]) for k in range(6)]
    assert widths == [1, 1, 2, 3, 5, 9], widths             # (this writer spends one bit on a dictionary of one entry)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_twin_equals_read_table(cases, name):
    c = cases[name]
    data = c.data
    want_table = pq.read_table(c.path)
    for k, cname in enumerate(want_table.column_names):
        vals, valid, strs = C.expected_column(want_table.column(cname))
        got_vals, got_valid, off, byts = hip.parquet_read_column_host(data, k)
        assert np.array_equal(got_valid, valid), cname
        if strs is None:
            assert off is None and np.array_equal(got_vals, vals), cname
        else:
            assert got_vals is None and off[0] == 0 and off[-1] == len(byts) == sum(len(s) for s in strs), cname
            assert [byts[off[i]:off[i + 1]] for i in range(len(strs))] == strs, cname


def test_overrides_on_the_host(cases):
    c = cases["matrix_decint_3groups"]
    data, names = c.data, c.table.column_names
    want = {n: C.expected_column(c.table.column(n)) for n in names}
    k32, k64 = names.index("i32_n"), names.index("i64_r")
    v, valid, _o, _b = hip.parquet_read_column_host(data, k32, hip.PH_I64)
    assert np.array_equal(v, want["i32_n"][0]) and np.array_equal(valid, want["i32_n"][1])
    v, _valid, _o, _b = hip.parquet_read_column_host(data, k32, hip.PH_DEC64, 3)
    assert np.array_equal(v, want["i32_n"][0])
    v, _valid, _o, _b = hip.parquet_read_column_host(data, k64, hip.PH_DEC64, 18)
    assert np.array_equal(v, want["i64_r"][0])
    with pytest.raises(hip.PlanHipError) as e:                 # the values leave int32
        hip.parquet_read_column_host(data, k64, hip.PH_I32)
    assert e.value.code == EOVERFLOW and "i64_r" in str(e.value) and "int32" in str(e.value)
    small = cases["dict_widths"]
    v, _valid, _o, _b = hip.parquet_read_column_host(small.data, 1, hip.PH_I32)     # d2: two small values, narrows
    assert np.array_equal(v, C.expected_column(small.table.column("d2"))[0])
    # naming the schema's own type is no override
    v, _valid, _o, _b = hip.parquet_read_column_host(data, names.index("d15_r"), hip.PH_DEC64, 2)
    assert np.array_equal(v, want["d15_r"][0])
    bad = [("i32_n", hip.PH_DATE, 0), ("i32_n", hip.PH_STR, 0), ("i32_n", hip.PH_DEC64, 19), ("i32_n", hip.PH_DEC64, -1), ("i32_n", hip.PH_F64, 0),
           ("date_n", hip.PH_I32, 0), ("date_n", hip.PH_I64, 0), ("date_r", hip.PH_DEC64, 0), ("d15_r", hip.PH_I64, 0), ("d15_r", hip.PH_DEC64, 3),
           ("d9_n", hip.PH_I32, 0), ("s40_n", hip.PH_I32, 0), ("s40_r", hip.PH_CODE8, 0), ("i64_r", hip.PH_DATE, 0), ("i64_r", 99, 0)]
    for cname, typ, scale in bad:
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, names.index(cname), typ, scale)
        assert e.value.code == EINVAL and cname in str(e.value), (cname, typ, scale, str(e.value))


def test_flba_decimal_outside_int64_overflows(files):
    import decimal
    t = pa.table({"ok": pa.array([decimal.Decimal(2**63 - 1), decimal.Decimal(-2**63), None], pa.decimal128(38, 0)),
                  "big": pa.array([decimal.Decimal(1), decimal.Decimal(2**63), None], pa.decimal128(38, 0)),
                  "neg": pa.array([decimal.Decimal(-2**63 - 1), None, None], pa.decimal128(38, 0)),
                  "wide": pa.array([decimal.Decimal(1)], pa.decimal128(38, 20)).take(pa.array([0, 0, 0]))})
    path = files / "flba16.parquet"
    pq.write_table(t, path, compression="NONE")
    data = path.read_bytes()
    v, valid, _o, _b = hip.parquet_read_column_host(data, 0)
    assert v.tolist() == [2**63 - 1, -2**63, 0] and valid.tolist() == [True, True, False]
    for k, cname in ((1, "big"), (2, "neg")):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, k)
        assert e.value.code == EOVERFLOW and cname in str(e.value)
    with pytest.raises(hip.PlanHipError) as e:                 # scale 20
        hip.parquet_read_column_host(data, 3)
    assert e.value.code == EUNSUPPORTED and "wide" in str(e.value)


def test_refusals_name_the_column_and_what_they_met(files):
    for name, (path, cname, word) in C.refusals(files).items():
        data = open(path, "rb").read()
        cols = [c["name"] for c in loader.parquet_schema(data)["columns"]]
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, cols.index(cname))
        assert e.value.code == EUNSUPPORTED and cname in str(e.value) and word in str(e.value), (name, str(e.value))
    # only the requested column is judged: the INT32 column beside the DOUBLE and the list reads
    path = C.refusals(files)["double"][0]
    v, _valid, _o, _b = hip.parquet_read_column_host(open(path, "rb").read(), 0)
    assert v.tolist() == list(range(100))
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(open(path, "rb").read(), 7)
    assert e.value.code == EINVAL


def test_host_checks_refuse_cut_and_mislabelled_files(cases):
    data = cases["matrix_decint_3groups"].data
    for name, bad in C.truncations(data).items():
        for call in (lambda: hip.parquet_schema(bad), lambda: hip.parquet_pages(bad, 0), lambda: hip.parquet_read_column_host(bad, 0)):
            with pytest.raises(hip.PlanHipError) as e:
                call()
            assert e.value.code == EINVAL, (name, str(e.value))


def test_offsets_and_sizes_in_the_footer_are_checked_against_the_file(cases):
    """a chunk offset, a chunk size or a page size that points outside the file (or its chunk) is PH_EINVAL before anything is decoded:
    the file is cut in front of the footer so that the footer's chunk ranges no longer fit"""
    data = cases["rows_65"].data
    flen = int.from_bytes(data[-8:-4], "little")
    footer = data[len(data) - 8 - flen:]
    for keep in (4, 40, 400):
        bad = data[:keep] + footer                      # the footer is intact, the chunks it names are gone
        assert hip.parquet_schema(bad)[0] == 65
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(bad, len(cases["rows_65"].table.column_names) - 1)
        assert e.value.code == EINVAL, str(e.value)
    # a page size beyond its chunk: the compressed_page_size varint of the first page header grows
    small = cases["rows_1"].data
    p = pages_of(small, 1)[0]
    hdr = small[p["header_pos"]:p["data_pos"]]
    assert hdr[0] == 0x15                                # field 1 (type), i32
    at = p["header_pos"] + 4                             # 0x15 <type> 0x15 <uncompressed, one byte> 0x15 <compressed, one byte>
    assert small[at - 2] == 0x15 and small[at] == 0x15 and small[at + 1] < 0x80 and small[at + 1] == small[at - 1]
    bad = small[:at + 1] + bytes([0xfe, 0xff, 0x7f]) + small[at + 2:]
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(bad, 1)
    assert e.value.code == EINVAL and "leaves its chunk" in str(e.value), str(e.value)


def test_one_byte_patches_only_decoding_can_see(files):
    for name, (orig, bad, column) in C.patched(files, pages_of).items():
        good = hip.parquet_read_column_host(orig, column)
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(bad, column)
        assert e.value.code == EINVAL and "row group 0, page" in str(e.value), (name, str(e.value))
        assert ("column %d (" % column) in str(e.value)
        # the patch hit what it meant to: pyarrow raises, or reads something else (but for the patches named "tolerated": stricter here than there)
        if name.startswith("tolerated"):
            continue
        try:
            theirs = pq.read_table(pa.BufferReader(bad))
        except Exception:  # noqa: BLE001
            continue
        assert not theirs.equals(pq.read_table(pa.BufferReader(orig))), name
        assert good is not None


SANITIZER_PROGRAM = r"""
#include "parquet_decode.h"
#include <cstdio>
#include <fstream>
#include <iterator>

// decodes every leaf column of every file named on the command line with the decoders the kernels instantiate; a refused file or column is
// fine (it is counted), a read out of range is the sanitizer's to report
int main(int argc, char **argv) {
    long decoded = 0, refused = 0;
    for (int a = 1; a < argc; a++) {
        std::ifstream in(argv[a], std::ios::binary);
        std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        std::vector<uint8_t> file(raw.begin(), raw.end());          // exactly nbytes: one byte past the end is out of range
        ph::pq::FileMeta fm;
        ph::pq::Status st;
        if (ph::pq::parse_footer(file.data(), (int64_t)file.size(), &fm, &st) != PH_OK) { refused++; continue; }
        for (size_t c = 0; c < fm.leaves.size(); c++) {
            for (int type : {0, (int)PH_I32, (int)PH_I64, (int)PH_DEC64}) {
                ph::pq::ColPlan cp;
                ph::pq::Status s2;
                if (ph::pq::resolve_column(file.data(), (int64_t)file.size(), fm, (int32_t)c, type, 2, &cp, &s2) != PH_OK || fm.num_rows >= (1ll << 31)) { refused++; continue; }
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
    }
    std::printf("decoded %ld refused %ld\n", decoded, refused);
    return 0;
}
"""


def test_decoders_under_address_sanitizer(cases, files, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the sanitizer check of the Parquet decoders needs a C++17 host compiler")
    src = tmp_path / "parquet_asan.cpp"
    src.write_text(SANITIZER_PROGRAM)
    exe = tmp_path / "parquet_asan"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         f"-I{ROOT / 'plan_amd' / 'csrc'}", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    paths = [c.path for c in cases.values()] + sorted({p for p, _c, _w in C.refusals(files).values()})
    bad_dir = tmp_path / "bad"
    bad_dir.mkdir()
    for name, (_orig, bad, _column) in C.patched(files, pages_of).items():
        (bad_dir / (name + ".parquet")).write_bytes(bad)
        paths.append(str(bad_dir / (name + ".parquet")))
    for name, bad in C.truncations(cases["matrix_decint_3groups"].data).items():
        (bad_dir / (name + ".parquet")).write_bytes(bad)
        paths.append(str(bad_dir / (name + ".parquet")))
    run = subprocess.run([str(exe)] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    decoded, refused = (int(x) for x in run.stdout.split()[1::2])
    assert decoded > 300 and refused > 20, run.stdout
