"""GZIP pages of the Parquet load path, without a GPU. The raw decoder (ph_gzip_decompress_host, the host instance of the
__host__ __device__ functions the inflate kernel instantiates) against the bit writer's model, zlib and pyarrow's gzip codec on crafted
streams — stored, fixed and dynamic blocks at the edges of their fields, members and header fields, fields across the kernel's input
window, an output that wraps its ring — on the corrupt ones with the sub-case each is refused for, on the two lists where this decoder
and pyarrow differ on purpose, and on zlib's own output. Then ph_parquet_pages_ex against pyarrow's metadata,
ph_parquet_read_column_host_ex with PH_PARQUET_GZIP against pq.read_table value by value on the files of tests/gzip_cases.py, the flag
matrix and the refusals (no flag, another codec, patches), and all of it once more in a stand-alone program under AddressSanitizer. Bytes
and integers: equality is the tolerance."""
import pathlib
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import pyarrow as pa
import pyarrow.parquet as pq

import gzip_cases as G
import parquet_cases as C
from plan_amd import hip, loader

ROOT = pathlib.Path(__file__).resolve().parents[1]
OK, EINVAL, EUNSUPPORTED = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED
SNAPPY, DELTA, LZ4_RAW = hip.PH_PARQUET_SNAPPY, hip.PH_PARQUET_DELTA, hip.PH_PARQUET_LZ4_RAW
GZIP = getattr(hip, "PH_PARQUET_GZIP", 64)
CODEC = pa.Codec("gzip")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("gzip_cases")


@pytest.fixture(scope="module")
def cases(files):
    return G.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column, codecs=True)


def theirs(stream, n):
    """pyarrow's gzip codec: the bytes, or None when it refuses the stream"""
    try:
        return CODEC.decompress(stream, decompressed_size=n).to_pybytes()
    except Exception:  # noqa: BLE001
        return None


def zlib_says(stream):
    """every member of the stream through zlib, all input consumed -> bytes, or None when zlib refuses it"""
    out = b""
    try:
        while stream:
            o = zlib.decompressobj(31)
            out += o.decompress(stream)
            if not o.eof:
                return None
            stream = o.unused_data
    except zlib.error:
        return None
    return out


def ours(stream, n):
    try:
        return hip.gzip_decompress_host(stream, n)
    except hip.PlanHipError as e:
        assert e.code == EINVAL and "corrupt GZIP stream" in str(e), str(e)
        return None


def test_window_and_ring_are_the_kernels():
    text = (ROOT / "plan_amd" / "csrc" / "gzip_decompress.h").read_text()
    assert int(re.search(r"constexpr int GZ_TILE = (\d+);", text).group(1)) == G.WINDOW
    assert int(re.search(r"constexpr int GZ_RING = (\d+);", text).group(1)) == G.RING
    (_name, stream, out), marks = G.straddling_stream()
    W = G.WINDOW
    assert marks == {"code": W - 1, "stored_len": 2 * W - 1, "dynamic_header": 3 * W - 5, "trailer": 4 * W - 3} and len(stream) > 4 * W
    assert stream[2 * W - 2] & 7 == 0 and stream[2 * W - 1:2 * W + 3] == bytes([300 & 255, 300 >> 8, ~300 & 255, (~300 >> 8) & 255])
    assert stream[4 * W - 3:4 * W + 5] == zlib.crc32(out[:-13]).to_bytes(4, "little") + (len(out) - 13).to_bytes(4, "little")
    assert stream[4 * W + 5:4 * W + 8] == b"\x1f\x8b\x08"


def test_the_case_lists_hold_what_the_issue_names():
    names = {n for n, _s, _o in G.valid_streams()}
    assert {"empty_fixed", "empty_stored", "stored_1", "stored_65535", "fixed_every_length_and_distance", "distance_1_times_1000000", "distance_equals_length",
            "distance_equals_produced", "ring_wraps_far_matches", "dynamic_15_bit_code_hlit_257_hdist_1", "dynamic_hlit_286_hdist_30",
            "dynamic_one_distance_code_of_1_bit", "dynamic_no_distance_code", "dynamic_repeat_codes_min_max", "dynamic_repeat_across_boundary", "three_block_types",
            "two_members", "three_members_empty_middle", "straddle_windows"} <= names
    assert {"stored_behind_%d_bits" % n for n in range(1, 8)} | {"header_" + n for n in ("fextra", "fname", "fcomment", "fhcrc", "all_fields")} <= names
    assert {"zlib_%s_level_%d" % (n, k) for n in ("text", "zeros", "random", "mix_900k") for k in (1, 6, 9)} <= names
    assert set(G.EVERY_LENGTH) >= {3, 4, 10, 11, 12, 257, 258} and len(G.EVERY_LENGTH) == 29 + 20
    _d, tokens, _seq = G.rle_tokens()
    assert {(16, 0), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)} <= set(tokens)
    words = {w for _n, _s, _e, w in G.invalid_streams()}
    assert len(words) == 18                                     # the 17 sub-cases of gzip_decode.h, the symbol one by both halves of its text
    assert len(G.stricter_streams()) == 2 and len(G.lenient_streams()) == 2


@pytest.mark.parametrize("case", G.valid_streams(), ids=lambda c: c[0])
def test_crafted_streams_inflate_as_the_model_zlib_and_pyarrow_say(case):
    _name, stream, out = case
    assert zlib_says(stream) == out and theirs(stream, len(out)) == out   # the writer and both references agree on what the stream says
    assert ours(stream, len(out)) == out


@pytest.mark.parametrize("case", G.invalid_streams(), ids=lambda c: c[0])
def test_corrupt_streams_are_refused_with_their_sub_case_and_by_zlib(case):
    name, stream, n, word = case
    z = zlib_says(stream)
    assert z is None or len(z) != n, name
    with pytest.raises(hip.PlanHipError) as e:
        hip.gzip_decompress_host(stream, n)
    assert e.value.code == EINVAL and "corrupt GZIP stream" in str(e.value) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("case", G.stricter_streams() + [G.RAW_DEFLATE], ids=lambda c: c[0])
def test_streams_refused_here(case):
    """zlib framing and output short of the expected length: pyarrow's codec reads both (a pyarrow that starts to refuse them shows up
    here); raw DEFLATE: it refuses that too"""
    name, stream, n, word = case
    assert (theirs(stream, n) is None) == (name == "raw_deflate"), name
    with pytest.raises(hip.PlanHipError) as e:
        hip.gzip_decompress_host(stream, n)
    assert e.value.code == EINVAL and "corrupt GZIP stream" in str(e.value) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("case", G.lenient_streams(), ids=lambda c: c[0])
def test_oddities_zlib_accepts_are_accepted(case):
    name, stream, out = case
    assert zlib_says(stream) == out and theirs(stream, len(out)) == out, name
    assert ours(stream, len(out)) == out


def test_sizes_the_host_refuses_before_it_decodes():
    assert hip.gzip_decompress_host(b"", 0) == b""
    empty = G.member(G.Deflate().fixed(final=True).end())
    assert len(empty) == 20 and hip.gzip_decompress_host(empty, 0) == b""
    for stream, n, word in ((b"", 1, "empty stream"), (empty[:19], 0, "fewer than the 20 bytes"), (empty, 20 * 1032 + 1, "1032")):
        with pytest.raises(hip.PlanHipError) as e:
            hip.gzip_decompress_host(stream, n)
        assert e.value.code == EINVAL and word in str(e.value), str(e.value)
    # 1032 to one is nearly reachable: 10 MB of zeros at level 9 come to more than 1000 to one and inflate
    n = 10000000
    z = G.gz(bytes(n), 9)
    assert 1000 * len(z) < n <= 1032 * len(z) and ours(z, n) == bytes(n)


def test_zlib_output_cut_and_extended():
    for name, data in G.roundtrip_inputs():
        stream = G.gz(data, 6)
        assert ours(stream[:-1], len(data)) is None and ours(stream + b"\0", len(data)) is None, name
        assert ours(stream, len(data) - 1) is None and ours(stream, len(data) + 1) is None, name


def test_case_list_is_complete(cases):
    assert sorted(G.CASE_NAMES) == sorted(cases)


def test_writer_knobs_gave_the_awkward_pages(cases):
    """the set holds what it is meant to, ph_parquet_pages_ex lists codec 2 and its sizes are the writer's"""
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
                assert cc.compression == "GZIP" and all(p["codec"] == 2 for p in mine)
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
                if p["compressed"] and p["uncompressed_bytes"] - levels > 800000 and p["data_bytes"] - levels > 3 * G.WINDOW:
                    seen.add("section of 900 KB")
                assert p["kind"] == hip.PH_PARQUET_PAGE_DATA_V2 or p["compressed"] == 1
        if md.num_row_groups > 1:
            seen.add("several row groups")
    assert seen == {"v1 compressed", "v1 all NULL", "v2 compressed", "v2 raw", "dictionary compressed", "section of 900 KB", "several row groups"}, seen
    # the plain entry point refuses these as before
    with pytest.raises(hip.PlanHipError) as e:
        loader.parquet_pages(cases["rows_65"].data, 0)
    assert e.value.code == EUNSUPPORTED and "GZIP" in str(e.value)


def check_column(data, k, col, flags, cname):
    vals, valid, strs = C.expected_column(col)
    got_vals, got_valid, off, byts = hip.parquet_read_column_host(data, k, flags=flags)
    assert np.array_equal(got_valid, valid), cname
    if strs is None:
        assert off is None and np.array_equal(got_vals, vals), cname
    else:
        assert got_vals is None and off[0] == 0 and off[-1] == len(byts) == sum(len(s) for s in strs), cname
        assert [byts[off[i]:off[i + 1]] for i in range(len(strs))] == strs, cname


REFUSAL_TAILS = {0: "only UNCOMPRESSED pages are decoded", 1: "only UNCOMPRESSED and SNAPPY pages are decoded", 5: "only UNCOMPRESSED and SNAPPY pages are decoded",
                 16: "only UNCOMPRESSED and LZ4_RAW pages are decoded", 21: "only UNCOMPRESSED, SNAPPY and LZ4_RAW pages are decoded"}


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_host_twin_equals_read_table(cases, name):
    c = cases[name]
    data = c.data
    want_table = pq.read_table(c.path)
    for k, cname in enumerate(want_table.column_names):
        check_column(data, k, want_table.column(cname), GZIP, cname)
        if c.table.num_rows:
            for flags, tail in REFUSAL_TAILS.items():              # without the flag: refused, in the words these flags always had
                with pytest.raises(hip.PlanHipError) as e:
                    hip.parquet_read_column_host(data, k, flags=flags)
                assert e.value.code == EUNSUPPORTED and "GZIP pages" in str(e.value) and cname in str(e.value) and str(e.value).endswith(tail), str(e.value)


@pytest.mark.parametrize("name", ["mixed_codecs", "delta_v1", "delta_v2"])
def test_mixed_codecs_and_delta_pages_in_gzip_chunks(files, name):
    c, more = G.flagged_files(files)[name]
    data = c.data
    want_table = pq.read_table(c.path)
    md = pq.ParquetFile(c.path).metadata
    codecs = {md.row_group(0).column(k).compression for k in range(md.num_columns)}
    assert codecs == ({"GZIP", "SNAPPY", "LZ4", "UNCOMPRESSED"} if name == "mixed_codecs" else {"GZIP"}) and md.num_row_groups >= (1 if name == "delta_v2" else 3)
    if name != "mixed_codecs":
        assert any("DELTA_BINARY_PACKED" in md.row_group(0).column(k).encodings for k in range(md.num_columns))
    for k, cname in enumerate(want_table.column_names):
        check_column(data, k, want_table.column(cname), GZIP | more, cname)
    # with a flag missing the columns in its domain are refused, the rest reads
    if name == "mixed_codecs":
        for flags, codec in ((GZIP | LZ4_RAW, "SNAPPY"), (GZIP | SNAPPY, "LZ4_RAW"), (SNAPPY | LZ4_RAW, "GZIP")):
            refused = 0
            for k, cname in enumerate(want_table.column_names):
                if G.MIXED_CODECS[cname] == codec:
                    with pytest.raises(hip.PlanHipError) as e:
                        hip.parquet_read_column_host(data, k, flags=flags)
                    assert e.value.code == EUNSUPPORTED and codec + " pages" in str(e.value)
                    refused += 1
                else:
                    check_column(data, k, want_table.column(cname), flags, cname)
            assert refused >= 3


def test_flag_matrix(cases, files):
    gz = cases["rows_65"].data
    for flags in (32, 96, 128, 2, 66, 72, 0x80000000):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(gz, 0, flags=flags)
        assert e.value.code == EINVAL and all(w in str(e.value) for w in ("flags", "PH_PARQUET_SNAPPY", "PH_PARQUET_DELTA", "PH_PARQUET_LZ4_RAW", "PH_PARQUET_GZIP")), str(e.value)
    plain = C._write(files, "gz_none_flag", cases["rows_65"].table)
    for flags in (64, 65, 68, 80, 85):
        for k in (0, 3, 11):
            a, b = hip.parquet_read_column_host(gz, k, flags=flags), hip.parquet_read_column_host(plain.data, k)
            assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
    for k in (0, 3, 11):                                           # word 64 on an uncompressed file reads as flags 0
        a, b = hip.parquet_read_column_host(plain.data, k, flags=64), hip.parquet_read_column_host(plain.data, k)
        assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
    for flags, tail in REFUSAL_TAILS.items():
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(gz, 0, flags=flags)
        assert e.value.code == EUNSUPPORTED and "GZIP pages" in str(e.value) and str(e.value).endswith(tail)
    assert {p["codec"] for p in pages_of(gz, 0)} == {2}


def test_other_codecs_are_refused_with_the_flag_too(files):
    t = pa.table({"i": pa.array(np.arange(100, dtype=np.int32))})
    zs = C._write(files, "gz_refuse_zstd", t, compression="ZSTD").data
    for flags, text in ((GZIP, "only UNCOMPRESSED and GZIP pages are decoded"), (GZIP | SNAPPY, "only UNCOMPRESSED, SNAPPY and GZIP pages are decoded"),
                        (GZIP | LZ4_RAW, "only UNCOMPRESSED, LZ4_RAW and GZIP pages are decoded"),
                        (GZIP | SNAPPY | LZ4_RAW | DELTA, "only UNCOMPRESSED, SNAPPY, LZ4_RAW and GZIP pages are decoded")):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(zs, 0, flags=flags)
        assert e.value.code == EUNSUPPORTED and "ZSTD pages" in str(e.value) and "(i)" in str(e.value) and str(e.value).endswith(text), str(e.value)
    if pa.Codec.is_available("brotli"):
        br = C._write(files, "gz_refuse_brotli", t, compression="BROTLI").data
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(br, 0, flags=GZIP)
        assert e.value.code == EUNSUPPORTED and "BROTLI pages" in str(e.value)
    for codec, name in (("SNAPPY", "SNAPPY"), ("LZ4_RAW", "LZ4_RAW")):
        data = C._write(files, "gz_refuse_" + name.lower(), t, compression=codec).data
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, 0, flags=GZIP)
        assert e.value.code == EUNSUPPORTED and name + " pages" in str(e.value) and str(e.value).endswith("only UNCOMPRESSED and GZIP pages are decoded")


def test_patches(files):
    for name, (orig, bad, column, page, word) in G.patched(files, pages_of).items():
        good = hip.parquet_read_column_host(orig, column, flags=GZIP)
        assert good[0] is not None
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(bad, column, flags=GZIP)
        msg = str(e.value)
        assert e.value.code == EINVAL and ("column %d (" % column) in msg and ("row group 0, page %d:" % page) in msg and word in msg, (name, msg)
        try:                                                       # the patch hit what it meant to: pyarrow raises or reads something else
            other = pq.read_table(pa.BufferReader(bad))
        except Exception:  # noqa: BLE001
            continue
        assert not other.equals(pq.read_table(pa.BufferReader(orig))), name
    both, column = G.two_bad_pages(files, pages_of)
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(both, column, flags=GZIP)
    assert e.value.code == EINVAL and "page 1: a corrupt GZIP stream" in str(e.value)


SANITIZER_PROGRAM = r"""
#include "parquet_decode.h"
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

// argv: files. *.stream = an 8-byte little-endian expected length, then ONE GZIP stream: inflated into a buffer of exactly that length
// from a buffer of exactly the stream's length. Everything else = a Parquet file: every leaf column resolved and decoded with
// every flag by the functions the kernels instantiate. A refused input is fine (it is counted), a read or write out of range is the
// sanitizer's to report.
static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream in(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    return std::vector<uint8_t>(raw.begin(), raw.end());
}

int main(int argc, char **argv) {
    long decoded = 0, refused = 0;
    const uint32_t flags = PH_PARQUET_GZIP | PH_PARQUET_LZ4_RAW | PH_PARQUET_SNAPPY | PH_PARQUET_DELTA;
    for (int a = 1; a < argc; a++) {
        const std::string path = argv[a];
        std::vector<uint8_t> file = slurp(argv[a]);                 // exactly nbytes: one byte past the end is out of range
        if (path.size() > 7 && path.compare(path.size() - 7, 7, ".stream") == 0) {
            int64_t expected = 0;
            memcpy(&expected, file.data(), 8);
            if (expected > (1ll << 30)) { refused++; continue; }   // (what check_sizes refuses anyway: nothing is allocated for it)
            std::vector<uint8_t> stream(file.begin() + 8, file.end()), out((size_t)expected);
            if (ph::gzip::decompress_host(stream.data(), (int64_t)stream.size(), out.data(), expected) != ph::gzip::S_OK) refused++;
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
        pytest.fail("g++ not found: the sanitizer check of the GZIP decoder needs a C++17 host compiler")
    src = tmp_path / "gzip_asan.cpp"
    src.write_text(SANITIZER_PROGRAM)
    exe = tmp_path / "gzip_asan"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         f"-I{ROOT / 'plan_amd' / 'csrc'}", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    good = [(name, stream, len(out)) for name, stream, out in G.valid_streams() + G.lenient_streams()]
    bad = [c[:3] for c in G.invalid_streams() + G.stricter_streams() + [G.RAW_DEFLATE]]
    paths = []
    for name, stream, n in good + bad:
        p = tmp_path / (name + ".stream")
        p.write_bytes(int(n).to_bytes(8, "little") + stream)
        paths.append(str(p))
    flagged = G.flagged_files(files)
    paths += [c.path for c in cases.values()] + [c.path for c, _more in flagged.values()] + G.write_patched(tmp_path, pages_of)
    both, _column = G.two_bad_pages(files, pages_of)
    (tmp_path / "two_bad.parquet").write_bytes(both)
    paths.append(str(tmp_path / "two_bad.parquet"))
    ncols = sum(c.table.num_columns for c in cases.values()) + sum(c.table.num_columns for c, _more in flagged.values())
    run = subprocess.run([str(exe)] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    decoded, refused = (int(x) for x in run.stdout.split()[1::2])
    # (every patched file holds one column)
    assert decoded == len(good) + ncols and refused == len(bad) + len(G.patched(files, pages_of)) + 1, run.stdout
