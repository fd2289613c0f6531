"""SNAPPY pages of the Parquet load path, without a GPU. The raw decoder (ph_snappy_decompress_host, the host instance of the
__host__ __device__ functions the decompression kernel shares) against pyarrow's Snappy on crafted streams — every element form, overlapping
and far copies, elements across the kernel's input tile, and the corrupt ones — and on Codec.compress output. Then ph_parquet_pages_ex
against pyarrow's metadata, ph_parquet_read_column_host_ex with PH_PARQUET_SNAPPY against pq.read_table value by value on the files of
tests/snappy_cases.py, the refusals (no flag, another codec, one-byte patches), and all of it once more in a stand-alone program under
AddressSanitizer. Bytes and integers: equality is the tolerance."""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")
if not pa.Codec.is_available("snappy"):
    pytest.skip("this pyarrow has no Snappy codec", allow_module_level=True)

import parquet_cases as C  # noqa: E402
import snappy_cases as S  # noqa: E402
from plan_amd import hip, loader  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parents[1]
OK, EINVAL, EUNSUPPORTED = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED
SNAPPY = hip.PH_PARQUET_SNAPPY
CODEC = pa.Codec("snappy")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("snappy_cases")


@pytest.fixture(scope="module")
def cases(files):
    return S.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column, codecs=True)


def theirs(stream, n):
    """pyarrow's Snappy: the bytes, or None when it refuses the stream"""
    try:
        return CODEC.decompress(stream, decompressed_size=n).to_pybytes()
    except Exception:  # noqa: BLE001
        return None


def ours(stream, n):
    try:
        return hip.snappy_decompress_host(stream, n)
    except hip.PlanHipError as e:
        assert e.code == EINVAL, str(e)
        return None


def test_tile_and_ring_are_the_kernels():
    text = (ROOT / "plan_amd" / "csrc" / "snappy_decompress.h").read_text()
    assert int(re.search(r"constexpr int SN_TILE = (\d+);", text).group(1)) == S.TILE
    assert int(re.search(r"constexpr int SN_RING = (\d+);", text).group(1)) == S.RING
    (_name, stream, _out), marks = S.straddling_stream()
    assert marks == [S.TILE - 1, 2 * S.TILE - 2, 3 * S.TILE - 3] and len(stream) > 3 * S.TILE
    by_pos = {e[0]: e for e in S.elements(stream)}
    assert by_pos[marks[0]][1] == 2 and by_pos[marks[1]][:2] == (marks[1], 0) and by_pos[marks[1]][3] == 2 * S.TILE + 1 and by_pos[marks[2]][1] == 4


@pytest.mark.parametrize("case", S.valid_streams(), ids=lambda c: c[0])
def test_crafted_streams_decode_as_pyarrow_decodes_them(case):
    _name, stream, out = case
    assert theirs(stream, len(out)) == out                      # the builder and the reference agree on what the stream says
    assert ours(stream, len(out)) == out
    assert hip.snappy_decompress_host(stream) == out            # the length from the preamble


@pytest.mark.parametrize("case", S.invalid_streams(), ids=lambda c: c[0])
def test_corrupt_streams_are_refused_as_pyarrow_refuses_them(case):
    name, stream, n = case
    assert theirs(stream, n) is None, name
    with pytest.raises(hip.PlanHipError) as e:
        hip.snappy_decompress_host(stream, n)
    assert e.value.code == EINVAL and "corrupt Snappy stream" in str(e.value), str(e.value)


@pytest.mark.parametrize("case", S.stricter_streams(), ids=lambda c: c[0])
def test_a_preamble_below_the_expected_length_is_refused_too(case):
    _name, stream, n = case
    assert theirs(stream, n) is not None                        # (pyarrow takes n as room, not as the length)
    assert ours(stream, n) is None


def test_the_message_names_the_sub_case():
    want = {"offset_0": "offset 0", "offset_one_beyond_produced": "beyond the bytes produced", "literal_cut": "runs past the input",
            "literal_4_byte_length_cut": "runs past the input", "copy_operand_cut": "runs past the input", "copy_one_byte_past_expected": "past the expected length",
            "input_one_byte_short": "ends before the expected length", "one_element_too_many": "left over", "preamble_6_bytes": "preamble",
            "preamble_disagrees_larger": "preamble"}
    by = {name: (stream, n) for name, stream, n in S.invalid_streams() + S.stricter_streams()}
    for name, word in want.items():
        with pytest.raises(hip.PlanHipError) as e:
            hip.snappy_decompress_host(*by[name])
        assert word in str(e.value), (name, str(e.value))
    # a preamble no stream of this size can honour is refused before anything is allocated for it
    with pytest.raises(hip.PlanHipError) as e:
        hip.snappy_decompress_host(S.varint(23 * 7) + bytes(4))
    assert e.value.code == EINVAL and "22" in str(e.value)


def test_compressor_output_round_trips():
    for name, data in S.roundtrip_inputs():
        stream = CODEC.compress(data).to_pybytes()
        assert ours(stream, len(data)) == data, name
        if len(data) > 64:
            assert ours(stream[:-1], len(data)) is None and ours(stream + b"\0", len(data)) is None, name


def test_case_list_is_complete(cases):
    assert sorted(S.CASE_NAMES) == sorted(cases)


def test_writer_knobs_gave_the_awkward_pages(cases):
    """the set holds what it is meant to, and ph_parquet_pages_ex's sizes are the writer's: per chunk the stored bytes plus headers sum to
    total_compressed_size and the uncompressed sizes plus headers to total_uncompressed_size"""
    seen = set()
    for name, c in cases.items():
        md = pq.ParquetFile(c.path).metadata
        data = c.data
        for k in range(md.num_columns):
            pages = pages_of(data, k)
            for g in range(md.num_row_groups):
                cc = md.row_group(g).column(k)
                mine = [p for p in pages if p["row_group"] == g]
                if md.row_group(g).num_rows == 0 and not mine:
                    continue
                assert cc.compression == "SNAPPY" and all(p["codec"] == 1 for p in mine)
                assert sum(p["data_pos"] - p["header_pos"] + p["data_bytes"] for p in mine) == cc.total_compressed_size, (name, k, g)
                assert sum(p["data_pos"] - p["header_pos"] + p["uncompressed_bytes"] for p in mine) == cc.total_uncompressed_size, (name, k, g)
            for p in pages:
                levels = p["rep_levels_bytes"] + p["def_levels_bytes"]
                if p["kind"] == hip.PH_PARQUET_PAGE_DATA and p["compressed"]:
                    seen.add("v1 compressed")
                    if p["data_bytes"] > p["uncompressed_bytes"]:
                        seen.add("v1 grown")
                if p["kind"] == hip.PH_PARQUET_PAGE_DATA_V2:
                    seen.add("v2 compressed" if p["compressed"] else "v2 raw")
                    if not p["compressed"]:
                        assert p["data_bytes"] == p["uncompressed_bytes"]
                    if p["data_bytes"] == levels:
                        seen.add("v2 no value bytes")
                if p["kind"] == hip.PH_PARQUET_PAGE_DICTIONARY and p["compressed"]:
                    seen.add("dictionary compressed")
                if p["compressed"] and p["uncompressed_bytes"] - levels > S.RING and p["data_bytes"] - levels > S.TILE:
                    seen.add("section above the ring")
                assert p["kind"] == hip.PH_PARQUET_PAGE_DATA_V2 or p["compressed"] == 1
    assert seen == {"v1 compressed", "v1 grown", "v2 compressed", "v2 raw", "v2 no value bytes", "dictionary compressed", "section above the ring"}, seen
    # the plain entry point lists uncompressed chunks as before and refuses these
    with pytest.raises(hip.PlanHipError) as e:
        loader.parquet_pages(cases["rows_65"].data, 0)
    assert e.value.code == EUNSUPPORTED and "SNAPPY" in str(e.value)
    plain = C._write(pathlib.Path(cases["rows_65"].path).parent, "sn_none", cases["rows_65"].table)
    both = loader.parquet_pages(plain.data, 3, codecs=True)
    assert [{k: v for k, v in p.items() if k not in ("codec", "compressed", "uncompressed_bytes")} for p in both] == loader.parquet_pages(plain.data, 3)
    assert all(p["codec"] == 0 and p["compressed"] == 0 and p["uncompressed_bytes"] == p["data_bytes"] for p in both)


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_host_twin_equals_read_table(cases, name):
    c = cases[name]
    data = c.data
    want_table = pq.read_table(c.path)
    for k, cname in enumerate(want_table.column_names):
        vals, valid, strs = C.expected_column(want_table.column(cname))
        got_vals, got_valid, off, byts = hip.parquet_read_column_host(data, k, flags=SNAPPY)
        assert np.array_equal(got_valid, valid), cname
        if strs is None:
            assert off is None and np.array_equal(got_vals, vals), cname
        else:
            assert got_vals is None and off[0] == 0 and off[-1] == len(byts) == sum(len(s) for s in strs), cname
            assert [byts[off[i]:off[i + 1]] for i in range(len(strs))] == strs, cname
        if c.table.num_rows:
            with pytest.raises(hip.PlanHipError) as e:             # without the flag: refused as before
                hip.parquet_read_column_host(data, k)
            assert e.value.code == EUNSUPPORTED and "SNAPPY" in str(e.value) and cname in str(e.value)


def test_flags_and_other_codecs(cases, files):
    data = cases["rows_65"].data
    for flags in (2, 3, 0x80000000):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, 0, flags=flags)
        assert e.value.code == EINVAL and "flags" in str(e.value)
    # an uncompressed file reads the same with the flag
    plain = C._write(files, "sn_none_flag", cases["rows_65"].table)
    for k in (0, 3, 11):
        a, b = hip.parquet_read_column_host(plain.data, k), hip.parquet_read_column_host(plain.data, k, flags=SNAPPY)
        assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def test_a_gzip_file_is_refused_with_the_flag_too(files):
    if not pa.Codec.is_available("gzip"):
        pytest.skip("this pyarrow has no GZIP codec to write the file with")
    gz = open(S.write_gzip(files), "rb").read()
    for flags in (0, SNAPPY):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(gz, 0, flags=flags)
        assert e.value.code == EUNSUPPORTED and "GZIP" in str(e.value) and "(i)" in str(e.value)
    assert {p["codec"] for p in pages_of(gz, 0)} == {2}            # (listed all the same)


def test_one_byte_patches(files):
    for name, (orig, bad, column, page) in S.patched(files, pages_of).items():
        good = hip.parquet_read_column_host(orig, column, flags=SNAPPY)
        assert good[0] is not None or good[3]                     # (the unpatched file reads: values, or a VARCHAR column's bytes)
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(bad, column, flags=SNAPPY)
        msg = str(e.value)
        assert e.value.code == EINVAL and ("column %d (" % column) in msg and ("row group 0, page %d:" % page) in msg, (name, msg)
        if name.startswith("copy_offset_0") or name.startswith("dictionary_stream"):
            assert "corrupt SNAPPY stream" in msg
        if name.startswith("level_prefix"):
            assert "a level section of" in msg
        if name.startswith("uncompressed_size"):
            assert "22" in msg
        try:                                                       # the patch hit what it meant to: pyarrow raises or reads something else
            other = pq.read_table(pa.BufferReader(bad))
        except Exception:  # noqa: BLE001
            continue
        assert not other.equals(pq.read_table(pa.BufferReader(orig))), name
    both, column = S.two_bad_pages(files, pages_of)
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(both, column, flags=SNAPPY)
    assert e.value.code == EINVAL and "page 1:" in str(e.value)
    # a corrupt dictionary page and a corrupt data page: planhip.h's order of pages (a fixed-width dictionary's stream is judged last)
    for column, page in ((0, 2), (1, 0)):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(S.bad_dictionary_and_data_page(files, pages_of, column), column, flags=SNAPPY)
        assert e.value.code == EINVAL and ("page %d: a corrupt SNAPPY stream" % page) in str(e.value), (column, str(e.value))


SANITIZER_PROGRAM = r"""
#include "parquet_decode.h"
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

// argv: files. *.stream = an 8-byte little-endian expected length, then ONE raw Snappy stream: decoded into a buffer of exactly that length
// from a buffer of exactly the stream's length. Everything else = a Parquet file: every leaf column resolved and decoded with
// PH_PARQUET_SNAPPY by the functions the kernels instantiate. A refused input is fine (it is counted), a read or write out of range is the
// sanitizer's to report.
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
            int64_t expected = 0;
            memcpy(&expected, file.data(), 8);
            std::vector<uint8_t> stream(file.begin() + 8, file.end()), out((size_t)expected);
            int64_t len = 0;
            if (ph::snappy::decompress_host(stream.data(), (int64_t)stream.size(), out.data(), expected, &len) != ph::snappy::S_OK) refused++;
            else decoded++;
            continue;
        }
        ph::pq::FileMeta fm;
        ph::pq::Status st;
        if (ph::pq::parse_footer(file.data(), (int64_t)file.size(), &fm, &st) != PH_OK) { refused++; continue; }
        for (size_t c = 0; c < fm.leaves.size(); c++) {
            ph::pq::ColPlan cp;
            ph::pq::Status s2;
            if (ph::pq::resolve_column(file.data(), (int64_t)file.size(), fm, (int32_t)c, 0, 0, &cp, &s2, PH_PARQUET_SNAPPY) != PH_OK || fm.num_rows >= (1ll << 31)) { refused++; continue; }
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
        pytest.fail("g++ not found: the sanitizer check of the Snappy decoder needs a C++17 host compiler")
    src = tmp_path / "snappy_asan.cpp"
    src.write_text(SANITIZER_PROGRAM)
    exe = tmp_path / "snappy_asan"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         f"-I{ROOT / 'plan_amd' / 'csrc'}", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    paths = []
    streams = [(name, stream, len(out)) for name, stream, out in S.valid_streams()] + S.invalid_streams() + S.stricter_streams()
    streams += [(name, CODEC.compress(data).to_pybytes(), len(data)) for name, data in S.roundtrip_inputs()]
    for name, stream, n in streams:
        p = tmp_path / (name + ".stream")
        p.write_bytes(int(n).to_bytes(8, "little") + stream)
        paths.append(str(p))
    nvalid = len(streams) - len(S.invalid_streams()) - len(S.stricter_streams())
    paths += [c.path for c in cases.values()] + S.write_patched(tmp_path, pages_of)
    both, _column = S.two_bad_pages(files, pages_of)
    (tmp_path / "two_bad.parquet").write_bytes(both)
    paths.append(str(tmp_path / "two_bad.parquet"))
    for column in (0, 1):
        (tmp_path / ("dict_and_data_%d.parquet" % column)).write_bytes(S.bad_dictionary_and_data_page(files, pages_of, column))
        paths.append(str(tmp_path / ("dict_and_data_%d.parquet" % column)))
    ncols = sum(c.table.num_columns for c in cases.values())
    run = subprocess.run([str(exe)] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    decoded, refused = (int(x) for x in run.stdout.split()[1::2])
    # (the dictionary file has two columns, one of them patched: 2 patched files and the 2 with two bad pages decode their other column)
    assert decoded == nvalid + ncols + 4 and refused == len(S.invalid_streams()) + len(S.stricter_streams()) + len(S.patched(files, pages_of)) + 1 + 2, run.stdout
