"""LZ4_RAW pages of the Parquet load path, without a GPU. The raw decoder (ph_lz4_decompress_host, the host instance of the
__host__ __device__ functions the decompression kernel instantiates) against the builder's model and pyarrow's lz4_raw codec on crafted
blocks — every length form, overlapping and far matches, sequence headers across the kernel's input window, an output that wraps its ring —
on the corrupt ones, on the two lists where this decoder and liblz4 differ on purpose, and on Codec.compress output. Then
ph_parquet_pages_ex against pyarrow's metadata, ph_parquet_read_column_host_ex with PH_PARQUET_LZ4_RAW against pq.read_table value by value
on the files of tests/lz4_cases.py, the flag matrix and the refusals (no flag, another codec, one-byte patches), and all of it once more in
a stand-alone program under AddressSanitizer. Bytes and integers: equality is the tolerance."""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import pyarrow as pa
import pyarrow.parquet as pq

import lz4_cases as L
import parquet_cases as C
from plan_amd import hip, loader

ROOT = pathlib.Path(__file__).resolve().parents[1]
OK, EINVAL, EUNSUPPORTED = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED
SNAPPY, DELTA, LZ4_RAW = hip.PH_PARQUET_SNAPPY, hip.PH_PARQUET_DELTA, hip.PH_PARQUET_LZ4_RAW
CODEC = pa.Codec("lz4_raw")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("lz4_cases")


@pytest.fixture(scope="module")
def cases(files):
    return L.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column, codecs=True)


def theirs(stream, n):
    """pyarrow's lz4_raw (liblz4): the bytes, or None when it refuses the block"""
    try:
        return CODEC.decompress(stream, decompressed_size=n).to_pybytes()
    except Exception:  # noqa: BLE001
        return None


def ours(stream, n):
    try:
        return hip.lz4_decompress_host(stream, n)
    except hip.PlanHipError as e:
        assert e.code == EINVAL and "corrupt LZ4_RAW stream" in str(e), str(e)
        return None


def test_window_and_ring_are_the_kernels():
    text = (ROOT / "plan_amd" / "csrc" / "lz4_decompress.h").read_text()
    assert int(re.search(r"constexpr int LZ_TILE = (\d+);", text).group(1)) == L.WINDOW
    assert int(re.search(r"constexpr int LZ_RING = (\d+);", text).group(1)) == L.RING
    (_name, stream, out), marks = L.straddling_stream()
    W = L.WINDOW
    assert marks[:3] == [W - 1, 2 * W - 3, 3 * W - 12] and len(stream) > 3 * W
    by_pos = {s[0]: s for s in L.sequences(stream)}
    assert by_pos[marks[0]][1] == 20                                              # a token as the last byte of window 0
    assert by_pos[marks[1]][2] == 2 * W + 2 and stream[2 * W - 2:2 * W + 1] == b"\xff\xff\xff"   # an extension run across the end of window 1
    assert by_pos[marks[2]][3] == 3 * W - 1 and by_pos[marks[2]][4] == 0x1234     # offset bytes on either side of the end of window 2
    long_match = by_pos[marks[3]]
    assert long_match[4] == 1 and long_match[5] > 255 * W and stream[long_match[3] + 2:long_match[3] + 2 + W + 40] == b"\xff" * (W + 40)
    long_lit = by_pos[marks[4]]
    assert long_lit[2] // W + 2 == (long_lit[2] + long_lit[1]) // W               # a literal run that ends two windows after it began
    assert len(out) > 2 * L.RING


def test_the_case_lists_hold_what_the_issue_names():
    names = {n for n, _s, _o in L.valid_streams()}
    assert {"empty", "literal_1", "offset_1_times_1000000", "offset_equals_length", "offset_equals_produced", "far_matches_300", "straddle_windows", "ring_wraps"} <= names
    assert {"literal_%d" % n for n in (14, 15, 16, 269, 270, 65536)} | {"match_%d" % n for n in (4, 18, 19, 20, 273, 274)} <= names
    assert {"overlap_offset_%d" % n for n in (2, 3, 63, 64, 65)} | {"offset_%d" % n for n in (65472, 65473, 65535)} <= names
    assert len(L.invalid_streams()) >= 9 and len(L.stricter_streams()) >= 2 and len(L.lenient_streams()) == 3


@pytest.mark.parametrize("case", L.valid_streams(), ids=lambda c: c[0])
def test_crafted_blocks_decode_as_the_model_and_pyarrow_say(case):
    _name, stream, out = case
    assert theirs(stream, len(out)) == out                      # the builder and the reference agree on what the block says
    assert ours(stream, len(out)) == out


@pytest.mark.parametrize("case", L.invalid_streams(), ids=lambda c: c[0])
def test_corrupt_blocks_are_refused_as_pyarrow_refuses_them(case):
    name, stream, n, word = case
    assert theirs(stream, n) is None, name
    with pytest.raises(hip.PlanHipError) as e:
        hip.lz4_decompress_host(stream, n)
    assert e.value.code == EINVAL and "corrupt LZ4_RAW stream" in str(e.value) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("case", L.stricter_streams(), ids=lambda c: c[0])
def test_blocks_refused_here_and_read_by_pyarrow(case):
    """offset 0, and a block that produces fewer bytes than expected: a pyarrow that starts to refuse them shows up here"""
    name, stream, n, word = case
    assert theirs(stream, n) is not None, name
    with pytest.raises(hip.PlanHipError) as e:
        hip.lz4_decompress_host(stream, n)
    assert e.value.code == EINVAL and "corrupt LZ4_RAW stream" in str(e.value) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("case", L.lenient_streams(), ids=lambda c: c[0])
def test_blocks_read_here_and_refused_by_pyarrow(case):
    """the end-of-block restrictions bind compressors, not this decoder: a pyarrow that starts to read them shows up here"""
    name, stream, out = case
    assert theirs(stream, len(out)) is None, name
    assert ours(stream, len(out)) == out


def test_sizes_the_host_refuses_before_it_decodes():
    assert hip.lz4_decompress_host(b"", 0) == b"" and hip.lz4_decompress_host(b"\0", 0) == b""
    for stream, n, word in ((b"", 1, "empty stream"), (b"\x1f\x00\x01\x00\xff", 255 * 5 + 1, "255")):
        with pytest.raises(hip.PlanHipError) as e:
            hip.lz4_decompress_host(stream, n)
        assert e.value.code == EINVAL and word in str(e.value), str(e.value)
    # 255 to one is reachable: 1 000 006 zeros compress to fewer than 1 000 006 / 254 bytes
    z = CODEC.compress(bytes(1000006)).to_pybytes()
    assert 1000006 <= 255 * len(z) < 1000006 * 255 // 254 + 255 and ours(z, 1000006) == bytes(1000006)


def test_compressor_output_round_trips():
    for name, data in L.roundtrip_inputs():
        stream = CODEC.compress(data).to_pybytes()
        assert ours(stream, len(data)) == data, name
        if len(data) > 64:
            assert ours(stream[:-1], len(data)) is None and ours(stream + b"\0", len(data)) is None, name
            assert ours(stream, len(data) - 1) is None and ours(stream, len(data) + 1) is None, name


def test_case_list_is_complete(cases):
    assert sorted(L.CASE_NAMES) == sorted(cases)


def test_writer_knobs_gave_the_awkward_pages(cases):
    """the set holds what it is meant to, ph_parquet_pages_ex lists codec 7 and its sizes are the writer's"""
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
                assert cc.compression == "LZ4" and all(p["codec"] == 7 for p in mine)   # (pyarrow's name for codec 7; the footer's number is what ours lists)
                assert sum(p["data_pos"] - p["header_pos"] + p["data_bytes"] for p in mine) == cc.total_compressed_size, (name, k, g)
                assert sum(p["data_pos"] - p["header_pos"] + p["uncompressed_bytes"] for p in mine) == cc.total_uncompressed_size, (name, k, g)
            for p in pages:
                levels = p["rep_levels_bytes"] + p["def_levels_bytes"]
                if p["kind"] == hip.PH_PARQUET_PAGE_DATA and p["compressed"]:
                    seen.add("v1 compressed")
                    if name == "nulls_v1" and md.schema.column(k).name == "all_null":
                        seen.add("v1 all NULL")                    # a compressed page without a value byte
                if p["kind"] == hip.PH_PARQUET_PAGE_DATA_V2:
                    seen.add("v2 compressed" if p["compressed"] else "v2 raw")
                    if not p["compressed"]:
                        assert p["data_bytes"] == p["uncompressed_bytes"]
                if p["kind"] == hip.PH_PARQUET_PAGE_DICTIONARY and p["compressed"]:
                    seen.add("dictionary compressed")
                if p["compressed"] and p["uncompressed_bytes"] - levels > 800000 and p["data_bytes"] - levels > L.WINDOW:
                    seen.add("section of 900 KB")
                assert p["kind"] == hip.PH_PARQUET_PAGE_DATA_V2 or p["compressed"] == 1
        if md.num_row_groups > 1:
            seen.add("several row groups")
    assert seen == {"v1 compressed", "v1 all NULL", "v2 compressed", "v2 raw", "dictionary compressed", "section of 900 KB", "several row groups"}, seen
    # the plain entry point refuses these as before
    with pytest.raises(hip.PlanHipError) as e:
        loader.parquet_pages(cases["rows_65"].data, 0)
    assert e.value.code == EUNSUPPORTED and "LZ4_RAW" in str(e.value)


def check_column(data, k, col, flags, cname):
    vals, valid, strs = C.expected_column(col)
    got_vals, got_valid, off, byts = hip.parquet_read_column_host(data, k, flags=flags)
    assert np.array_equal(got_valid, valid), cname
    if strs is None:
        assert off is None and np.array_equal(got_vals, vals), cname
    else:
        assert got_vals is None and off[0] == 0 and off[-1] == len(byts) == sum(len(s) for s in strs), cname
        assert [byts[off[i]:off[i + 1]] for i in range(len(strs))] == strs, cname


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_host_twin_equals_read_table(cases, name):
    c = cases[name]
    data = c.data
    want_table = pq.read_table(c.path)
    for k, cname in enumerate(want_table.column_names):
        check_column(data, k, want_table.column(cname), LZ4_RAW, cname)
        if c.table.num_rows:
            for flags in (0, SNAPPY, SNAPPY | DELTA):              # without the flag: refused, in the words these flags always had
                with pytest.raises(hip.PlanHipError) as e:
                    hip.parquet_read_column_host(data, k, flags=flags)
                assert e.value.code == EUNSUPPORTED and "LZ4_RAW pages" in str(e.value) and cname in str(e.value)
                assert str(e.value).endswith("only UNCOMPRESSED and SNAPPY pages are decoded" if flags & SNAPPY else "only UNCOMPRESSED pages are decoded")


@pytest.mark.parametrize("name", ["mixed_codecs", "delta_v1", "delta_v2"])
def test_mixed_codecs_and_delta_pages_in_lz4_chunks(files, name):
    c, more = L.flagged_files(files)[name]
    data = c.data
    want_table = pq.read_table(c.path)
    md = pq.ParquetFile(c.path).metadata
    codecs = {md.row_group(0).column(k).compression for k in range(md.num_columns)}
    assert codecs == ({"SNAPPY", "LZ4", "UNCOMPRESSED"} if name == "mixed_codecs" else {"LZ4"}) and md.num_row_groups >= (1 if name == "delta_v2" else 3)
    if name != "mixed_codecs":
        assert any("DELTA_BINARY_PACKED" in md.row_group(0).column(k).encodings for k in range(md.num_columns))
    for k, cname in enumerate(want_table.column_names):
        check_column(data, k, want_table.column(cname), LZ4_RAW | more, cname)
    # with one of the two flags a column in the other's domain is refused, the rest reads
    if name == "mixed_codecs":
        for flags, codec in ((LZ4_RAW, "SNAPPY"), (SNAPPY, "LZ4_RAW")):
            refused = 0
            for k, cname in enumerate(want_table.column_names):
                if L.MIXED_CODECS[cname] == codec:
                    with pytest.raises(hip.PlanHipError) as e:
                        hip.parquet_read_column_host(data, k, flags=flags)
                    assert e.value.code == EUNSUPPORTED and codec + " pages" in str(e.value)
                    refused += 1
                else:
                    check_column(data, k, want_table.column(cname), flags, cname)
            assert refused >= 4


def test_flag_matrix(cases, files):
    lz = cases["rows_65"].data
    for flags in (2, 3, 6, 7, 8, 18, 24, 32, 0x80000000):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(lz, 0, flags=flags)
        assert e.value.code == EINVAL and all(w in str(e.value) for w in ("flags", "PH_PARQUET_SNAPPY", "PH_PARQUET_DELTA", "PH_PARQUET_LZ4_RAW")), str(e.value)
    plain = C._write(files, "lz_none_flag", cases["rows_65"].table)
    for flags in (16, 17, 20, 21):
        for k in (0, 3, 11):
            a, b = hip.parquet_read_column_host(lz, k, flags=flags), hip.parquet_read_column_host(plain.data, k)
            assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
    for k in (0, 3, 11):                                           # word 16 on an uncompressed file reads as flags 0
        a, b = hip.parquet_read_column_host(plain.data, k, flags=16), hip.parquet_read_column_host(plain.data, k)
        assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
    for flags in (0, 1, 5):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(lz, 0, flags=flags)
        assert e.value.code == EUNSUPPORTED and "LZ4_RAW" in str(e.value)
    assert {p["codec"] for p in pages_of(lz, 0)} == {7}


def test_other_codecs_are_refused_with_the_flag_too(files):
    t = pa.table({"i": pa.array(np.arange(100, dtype=np.int32))})
    gz = C._write(files, "lz_refuse_gzip", t, compression="GZIP").data
    for flags, text in ((LZ4_RAW, "only UNCOMPRESSED and LZ4_RAW pages are decoded"), (LZ4_RAW | SNAPPY, "only UNCOMPRESSED, SNAPPY and LZ4_RAW pages are decoded")):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(gz, 0, flags=flags)
        assert e.value.code == EUNSUPPORTED and "GZIP pages" in str(e.value) and "(i)" in str(e.value) and str(e.value).endswith(text), str(e.value)
    sn = C._write(files, "lz_refuse_snappy", t, compression="SNAPPY").data
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(sn, 0, flags=LZ4_RAW)
    assert e.value.code == EUNSUPPORTED and "SNAPPY pages" in str(e.value)
    # codec 5, the deprecated LZ4: no writer here produces it, so an LZ4_RAW file's footer is renumbered (the chunk's codec is the
    # one field of its metadata that holds 7 behind the field header 0x15: i32 field 4 follows field 3)
    lz = C._write(files, "lz_for_codec5", t, compression="LZ4_RAW").data
    flen = int.from_bytes(lz[-8:-4], "little")
    footer = lz[-8 - flen:-8]
    hits = [m.start() for m in re.finditer(rb"\x15\x0e", footer)]  # zigzag(7) = 14
    old = None
    for at in hits:
        cand = lz[:len(lz) - 8 - flen + at + 1] + b"\x0a" + lz[len(lz) - 8 - flen + at + 2:]   # zigzag(5) = 10
        try:
            got = {p["codec"] for p in pages_of(cand, 0)}
        except hip.PlanHipError:
            continue
        if got == {5}:
            old = cand
    assert old is not None
    for flags in (0, SNAPPY, LZ4_RAW, LZ4_RAW | SNAPPY | DELTA):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(old, 0, flags=flags)
        assert e.value.code == EUNSUPPORTED and "LZ4 pages" in str(e.value), str(e.value)
        assert ("deprecated" in str(e.value)) == bool(flags & LZ4_RAW)


def test_one_byte_patches(files):
    for name, (orig, bad, column, page, word) in L.patched(files, pages_of).items():
        good = hip.parquet_read_column_host(orig, column, flags=LZ4_RAW)
        assert good[0] is not None
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(bad, column, flags=LZ4_RAW)
        msg = str(e.value)
        assert e.value.code == EINVAL and ("column %d (" % column) in msg and ("row group 0, page %d:" % page) in msg and word in msg, (name, msg)
        try:                                                       # the patch hit what it meant to: pyarrow raises or reads something else
            other = pq.read_table(pa.BufferReader(bad))
        except Exception:  # noqa: BLE001
            continue
        assert not other.equals(pq.read_table(pa.BufferReader(orig))), name
    both, column = L.two_bad_pages(files, pages_of)
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(both, column, flags=LZ4_RAW)
    assert e.value.code == EINVAL and "page 1: a corrupt LZ4_RAW stream" in str(e.value)


SANITIZER_PROGRAM = r"""
#include "parquet_decode.h"
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

// argv: files. *.stream = an 8-byte little-endian expected length, then ONE bare LZ4 block: decoded into a buffer of exactly that length
// from a buffer of exactly the block's length. Everything else = a Parquet file: every leaf column resolved and decoded with
// PH_PARQUET_LZ4_RAW | PH_PARQUET_SNAPPY | PH_PARQUET_DELTA by the functions the kernels instantiate. A refused input is fine (it is
// counted), a read or write out of range is the sanitizer's to report.
static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream in(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    return std::vector<uint8_t>(raw.begin(), raw.end());
}

int main(int argc, char **argv) {
    long decoded = 0, refused = 0;
    const uint32_t flags = PH_PARQUET_LZ4_RAW | PH_PARQUET_SNAPPY | PH_PARQUET_DELTA;
    for (int a = 1; a < argc; a++) {
        const std::string path = argv[a];
        std::vector<uint8_t> file = slurp(argv[a]);                 // exactly nbytes: one byte past the end is out of range
        if (path.size() > 7 && path.compare(path.size() - 7, 7, ".stream") == 0) {
            int64_t expected = 0;
            memcpy(&expected, file.data(), 8);
            std::vector<uint8_t> stream(file.begin() + 8, file.end()), out((size_t)expected);
            if (ph::lz4::decompress_host(stream.data(), (int64_t)stream.size(), out.data(), expected) != ph::lz4::S_OK) refused++;
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
        pytest.fail("g++ not found: the sanitizer check of the LZ4 decoder needs a C++17 host compiler")
    src = tmp_path / "lz4_asan.cpp"
    src.write_text(SANITIZER_PROGRAM)
    exe = tmp_path / "lz4_asan"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         f"-I{ROOT / 'plan_amd' / 'csrc'}", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    good = [(name, stream, len(out)) for name, stream, out in L.valid_streams() + L.lenient_streams()]
    good += [(name, CODEC.compress(data).to_pybytes(), len(data)) for name, data in L.roundtrip_inputs()]
    bad = [c[:3] for c in L.invalid_streams() + L.stricter_streams()]
    paths = []
    for name, stream, n in good + bad:
        p = tmp_path / (name + ".stream")
        p.write_bytes(int(n).to_bytes(8, "little") + stream)
        paths.append(str(p))
    flagged = L.flagged_files(files)
    paths += [c.path for c in cases.values()] + [c.path for c, _more in flagged.values()] + L.write_patched(tmp_path, pages_of)
    both, _column = L.two_bad_pages(files, pages_of)
    (tmp_path / "two_bad.parquet").write_bytes(both)
    paths.append(str(tmp_path / "two_bad.parquet"))
    ncols = sum(c.table.num_columns for c in cases.values()) + sum(c.table.num_columns for c, _more in flagged.values())
    run = subprocess.run([str(exe)] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    decoded, refused = (int(x) for x in run.stdout.split()[1::2])
    # (every patched file holds one column)
    assert decoded == len(good) + ncols and refused == len(bad) + len(L.patched(files, pages_of)) + 1, run.stdout
