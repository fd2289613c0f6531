"""ZSTD pages of the Parquet load path, without a GPU. The raw decoder (ph_zstd_decompress_host, the host instance of the
__host__ __device__ functions the section kernel instantiates) against the stream writer's model and libzstd as pyarrow carries it, on
crafted streams — every header field, block type, literals type and size format, sequence mode, length and offset code, repeat-offset
rule, copies around the kernel's ring, fields across its input windows — on the corrupt ones with the sub-case each is refused for and
libzstd's verdict, on the list where this decoder is stricter on purpose, and on libzstd's own output at five levels. Then
ph_parquet_pages_ex against pyarrow's metadata, ph_parquet_read_column_host_ex with PH_PARQUET_ZSTD against pq.read_table value by value on
the files of tests/zstd_cases.py, the flag matrix and the refusals, and all of it once more in a stand-alone program under
AddressSanitizer. Bytes and integers: equality is the tolerance."""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import pyarrow as pa
import pyarrow.parquet as pq

import parquet_cases as C
import zstd_cases as Z
from plan_amd import hip, loader

ROOT = pathlib.Path(__file__).resolve().parents[1]
OK, EINVAL, EUNSUPPORTED = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED
SNAPPY, DELTA, LZ4_RAW, GZIP = hip.PH_PARQUET_SNAPPY, hip.PH_PARQUET_DELTA, hip.PH_PARQUET_LZ4_RAW, hip.PH_PARQUET_GZIP
ZSTD = getattr(hip, "PH_PARQUET_ZSTD", 256)
CODEC = pa.Codec("zstd")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("zstd_cases")


@pytest.fixture(scope="module")
def cases(files):
    return Z.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column, codecs=True)


def theirs(stream, n):
    """libzstd through pyarrow's codec: the bytes, or None when it refuses the stream (or the stream gives another length)"""
    try:
        return CODEC.decompress(stream, decompressed_size=n).to_pybytes()
    except Exception:  # noqa: BLE001
        return None


def ours(stream, n):
    try:
        return hip.zstd_decompress_host(stream, n)
    except hip.PlanHipError as e:
        assert e.code == EINVAL and "corrupt ZSTD stream" in str(e), str(e)
        return None


def test_window_and_ring_are_the_kernels():
    text = (ROOT / "plan_amd" / "csrc" / "zstd_decompress.h").read_text()
    assert int(re.search(r"constexpr int ZS_TILE = (\d+);", text).group(1)) == Z.WINDOW
    assert int(re.search(r"constexpr int ZS_RING = (\d+);", text).group(1)) == Z.RING
    assert "static_assert(ZS_LDS == 51776 && 3 * ZS_LDS <= 160 * 1024" in text
    _name, stream, out = Z.straddling_stream()
    # four literal streams and the sequence stream, each longer than a window
    at = stream.index(b"\x28\xb5\x2f\xfd") + 6 + 3 + 256 + 3
    v = int.from_bytes(stream[at:at + 5], "little")
    assert v & 3 == 2 and (v >> 2) & 3 == 3 and (v >> 4) & 0x3ffff == 14 * Z.WINDOW + 5
    tree = len(Z.tree_direct(Z.TEXT_WEIGHTS))
    sizes = [int.from_bytes(stream[at + 5 + tree + 2 * i:at + 7 + tree + 2 * i], "little") for i in range(3)]
    assert all(s > Z.WINDOW for s in sizes) and len(stream) - (at + 5 + ((v >> 22) & 0x3ffff)) > Z.WINDOW


def test_the_writer_s_xxh64_and_tables_are_libzstd_s():
    # a frame with a checksum that libzstd reads is a checksum libzstd computed the same way; one flipped bit is refused by both
    for n in (0, 1, 31, 32, 33, 100, 4133):
        data = Z.payload(n, n)
        stream, out = Z.one_frame(lambda f: f.raw(data, last=True), checksum=True)
        assert theirs(stream, n) == data == out
        assert theirs(stream[:-1] + bytes([stream[-1] ^ 1]), n) is None
    assert Z.xxh64(b"") == 0xef46db3751d8e999 and Z.xxh64(b"a") == 0xd24ec4f1a98c6e5b      # the published vectors of XXH64, seed 0


def test_the_case_lists_hold_what_the_issue_names():
    names = {n for n, _s, _o in Z.valid_streams()}
    assert {"empty_frame", "raw_0", "raw_1", "raw_131072", "rle_0", "rle_1", "rle_131072", "two_frames", "three_frames_empty_and_skippable_between",
            "literals_treeless_after_compressed", "literals_huffman_11_bit_code", "literals_huffman_fse_weights", "sequences_1", "sequences_127", "sequences_128",
            "sequences_32512", "sequences_every_length_code_base_and_top", "sequences_offset_codes_0_to_20", "sequences_repeat_offsets",
            "sequences_fse_compressed_tables", "sequences_rle_tables", "sequences_repeat_mode_after_fse_rle_and_predefined", "offset_1_times_1000000",
            "offset_equals_length", "offset_equals_produced", "offsets_around_the_ring", "far_match_into_unflushed_bytes", "far_match_of_100000",
            "straddle_windows"} <= names
    assert {"single_segment_fcs_%d%s" % (k, c) for k in (1, 2, 4, 8) for c in ("", "_checksum")} | {"window_fcs_%d%s" % (k, c) for k in (0, 2, 4, 8) for c in ("", "_checksum")} <= names
    assert {"literals_%s_fmt%d" % (k, f) for k in ("raw", "rle") for f in (0, 1, 3)} | {"literals_huffman_four_streams_fmt1_%d" % n for n in (37, 38, 39)} <= names
    assert any(len(o) > 4 * Z.RING for _n, _s, o in Z.valid_streams())
    # every sub-case of zstd_decode.h is met by a corrupt stream (two of them only on the stricter list)
    header = (ROOT / "plan_amd" / "csrc" / "zstd_decode.h").read_text()
    texts = re.findall(r'case S_[A-Z_]+: return "([^"]+)";', header)
    assert len(texts) == len(re.findall(r"^    S_[A-Z_]+ = \d+,", header, re.M)) - 1 > 20      # a text for every sub-case but S_OK
    met = set()
    for _n, stream, n, _w in Z.invalid_streams() + Z.stricter_streams():
        with pytest.raises(hip.PlanHipError) as e:
            hip.zstd_decompress_host(stream, n)
        met.add(str(e.value).split(": ")[-1] if "corrupt ZSTD stream" in str(e.value) else str(e.value))
    assert all(any(t in m for m in met) for t in texts), [t for t in texts if not any(t in m for m in met)]


@pytest.mark.parametrize("case", Z.valid_streams(), ids=lambda c: c[0])
def test_crafted_streams_decode_as_the_model_and_libzstd_say(case):
    _name, stream, out = case
    assert theirs(stream, len(out)) == out                       # the writer and the reference agree on what the stream says
    assert ours(stream, len(out)) == out


@pytest.mark.parametrize("case", Z.pyarrow_streams(), ids=lambda c: c[0])
def test_libzstd_output_decodes_and_is_refused_when_cut_extended_or_mis_sized(case):
    name, stream, data = case
    assert ours(stream, len(data)) == data
    assert ours(stream[:-1], len(data)) is None and ours(stream + b"\0", len(data)) is None, name
    assert ours(stream, len(data) - 1) is None and ours(stream, len(data) + 1) is None, name


def test_stream_statistics_account_for_every_byte():
    """ph_zstd_stream_stats_host: literal and match bytes make the output; a crafted frame's counts are the writer's"""
    _n, data = Z.pyarrow_inputs()[3]
    lits, seqs, match, far = hip.zstd_stream_stats_host(Z.zs(data, 19), len(data))
    assert lits + match == len(data) and seqs > 100 and 0 < far <= match        # (the mix repeats its text 400 KB later)
    stream, out = [(s, o) for n, s, o in Z.valid_streams() if n == "far_match_of_100000"][0]
    assert hip.zstd_stream_stats_host(stream, len(out)) == (2 * Z.RING, 2, 130000, 130000)
    assert hip.zstd_stream_stats_host(stream, len(out), far_limit=Z.RING + 16) == (2 * Z.RING, 2, 130000, 30000)


@pytest.mark.parametrize("case", [c for c in Z.invalid_streams() if "cut_at_" not in c[0] and not c[0].startswith("checksum_bit_")], ids=lambda c: c[0])
def test_corrupt_streams_are_refused_with_their_sub_case_and_by_libzstd(case):
    name, stream, n, word = case
    assert theirs(stream, n) is None, name
    with pytest.raises(hip.PlanHipError) as e:
        hip.zstd_decompress_host(stream, n)
    assert e.value.code == EINVAL and word in str(e.value), str(e.value)
    assert "corrupt ZSTD stream" in str(e.value)


def test_input_cut_at_every_byte_and_every_checksum_bit():
    many = [c for c in Z.invalid_streams() if "cut_at_" in c[0] or c[0].startswith("checksum_bit_")]
    good, out = Z.small_frame()
    assert theirs(good, len(out)) == out and ours(good, len(out)) == out
    assert len([c for c in many if c[0].startswith("cut_at_")]) == len(good) - 1 and len([c for c in many if c[0].startswith("checksum_bit_")]) == 32
    # the long header (18 bytes) and the second frame are cut at every byte of theirs, the checksum's four included
    assert len([c for c in many if c[0].startswith("long_header_cut_at_")]) == len([c for c in many if c[0].startswith("second_frame_cut_at_")]) == 18 + 3 + 6 + 4 - 1
    for name, stream, n, word in many:
        assert len(word) > 8, name                               # every one names its sub-case
        assert theirs(stream, n) is None, name
        with pytest.raises(hip.PlanHipError) as e:
            hip.zstd_decompress_host(stream, n)
        assert e.value.code == EINVAL and "corrupt ZSTD stream" in str(e.value) and word in str(e.value), (name, str(e.value))


@pytest.mark.parametrize("case", Z.stricter_streams(), ids=lambda c: c[0])
def test_streams_refused_here_and_read_by_libzstd(case):
    """a Huffman code of 12 bits and blocks above Block_Maximum_Size: libzstd's one-shot decoder reads them (a libzstd that starts to
    refuse them shows up here)"""
    name, stream, n, word = case
    assert theirs(stream, n) is not None, name
    with pytest.raises(hip.PlanHipError) as e:
        hip.zstd_decompress_host(stream, n)
    assert e.value.code == EINVAL and "corrupt ZSTD stream" in str(e.value) and word in str(e.value), str(e.value)


def test_sizes_the_host_refuses_before_it_decodes():
    assert hip.zstd_decompress_host(b"", 0) == b""
    empty, _o = Z.one_frame(lambda f: f.raw(b"", last=True))
    assert len(empty) == 9 and hip.zstd_decompress_host(empty, 0) == b""
    for stream, n, word in ((b"", 1, "empty stream"), (empty[:8], 0, "fewer than the 9 bytes"), (empty, 9 * 32768 + 1, "32768")):
        with pytest.raises(hip.PlanHipError) as e:
            hip.zstd_decompress_host(stream, n)
        assert e.value.code == EINVAL and word in str(e.value), str(e.value)
    # 32768 to one is nearly reachable: 10 MB of zeros at level 19 come to more than 30000 to one and decode
    n = 10000000
    z = Z.zs(bytes(n), 19)
    assert 30000 * len(z) < n <= 32768 * len(z) and ours(z, n) == bytes(n)


def test_case_list_is_complete(cases):
    assert sorted(Z.CASE_NAMES) == sorted(cases)


def test_writer_knobs_gave_the_awkward_pages(cases):
    """the set holds what it is meant to, ph_parquet_pages_ex lists codec 6 and its sizes are the writer's"""
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
                assert cc.compression == "ZSTD" and all(p["codec"] == 6 for p in mine)
                assert sum(p["data_pos"] - p["header_pos"] + p["data_bytes"] for p in mine) == cc.total_compressed_size, (name, k, g)
                assert sum(p["data_pos"] - p["header_pos"] + p["uncompressed_bytes"] for p in mine) == cc.total_uncompressed_size, (name, k, g)
            for p in pages:
                levels = p["rep_levels_bytes"] + p["def_levels_bytes"]
                if p["kind"] == hip.PH_PARQUET_PAGE_DATA and p["compressed"]:
                    seen.add("v1 compressed")
                if p["kind"] == hip.PH_PARQUET_PAGE_DATA_V2:
                    seen.add("v2 compressed" if p["compressed"] else "v2 raw")
                if p["kind"] == hip.PH_PARQUET_PAGE_DICTIONARY and p["compressed"]:
                    seen.add("dictionary compressed")
                if p["compressed"] and p["uncompressed_bytes"] - levels > 800000 and p["data_bytes"] - levels > 3 * Z.WINDOW:
                    seen.add("section of 900 KB")
        if md.num_row_groups > 1:
            seen.add("several row groups")
    assert seen >= {"v1 compressed", "v2 compressed", "dictionary compressed", "section of 900 KB", "several row groups"}, seen
    with pytest.raises(hip.PlanHipError) as e:                   # the plain entry point refuses these as before
        loader.parquet_pages(cases["rows_65"].data, 0)
    assert e.value.code == EUNSUPPORTED and "ZSTD" in str(e.value)


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
                 16: "only UNCOMPRESSED and LZ4_RAW pages are decoded", 21: "only UNCOMPRESSED, SNAPPY and LZ4_RAW pages are decoded",
                 64: "only UNCOMPRESSED and GZIP pages are decoded", 85: "only UNCOMPRESSED, SNAPPY, LZ4_RAW and GZIP pages are decoded"}


@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_host_twin_equals_read_table(cases, name):
    c = cases[name]
    data = c.data
    want_table = pq.read_table(c.path)
    for k, cname in enumerate(want_table.column_names):
        check_column(data, k, want_table.column(cname), ZSTD, cname)
    if c.table.num_rows:
        for flags, tail in REFUSAL_TAILS.items():                  # without the flag: refused, in the words these flags always had
            with pytest.raises(hip.PlanHipError) as e:
                hip.parquet_read_column_host(data, 0, flags=flags)
            assert e.value.code == EUNSUPPORTED and "ZSTD pages" in str(e.value) and str(e.value).endswith(tail), str(e.value)


@pytest.mark.parametrize("name", ["mixed_codecs", "delta_v1", "delta_v2"])
def test_mixed_codecs_and_delta_pages_in_zstd_chunks(files, name):
    c, more = Z.flagged_files(files)[name]
    data = c.data
    want_table = pq.read_table(c.path)
    md = pq.ParquetFile(c.path).metadata
    codecs = {md.row_group(0).column(k).compression for k in range(md.num_columns)}
    assert codecs == ({"ZSTD", "GZIP", "SNAPPY", "LZ4", "UNCOMPRESSED"} if name == "mixed_codecs" else {"ZSTD"})
    if name != "mixed_codecs":
        assert any("DELTA_BINARY_PACKED" in md.row_group(0).column(k).encodings for k in range(md.num_columns))
    for k, cname in enumerate(want_table.column_names):
        check_column(data, k, want_table.column(cname), ZSTD | more, cname)
    if name == "mixed_codecs":                                     # with a flag missing the columns in its domain are refused, the rest reads
        for flags, codec in ((ZSTD | GZIP | LZ4_RAW, "SNAPPY"), (GZIP | SNAPPY | LZ4_RAW, "ZSTD"), (ZSTD | SNAPPY | LZ4_RAW, "GZIP")):
            refused = 0
            for k, cname in enumerate(want_table.column_names):
                if Z.MIXED_CODECS[cname] == codec:
                    with pytest.raises(hip.PlanHipError) as e:
                        hip.parquet_read_column_host(data, k, flags=flags)
                    assert e.value.code == EUNSUPPORTED and codec + " pages" in str(e.value)
                    refused += 1
                else:
                    check_column(data, k, want_table.column(cname), flags, cname)
            assert refused >= 2


def test_flag_matrix(cases, files):
    zs = cases["rows_65"].data
    for flags in (256 | 2, 512, 256 | 8, 256 | 32, 256 | 128, 0x80000000):
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(zs, 0, flags=flags)
        assert e.value.code == EINVAL and all(w in str(e.value) for w in ("flags", "PH_PARQUET_SNAPPY", "PH_PARQUET_DELTA", "PH_PARQUET_LZ4_RAW", "PH_PARQUET_GZIP"))
        assert str(e.value).endswith("and PH_PARQUET_ZSTD are defined"), str(e.value)
    plain = C._write(files, "zs_none_flag", cases["rows_65"].table)
    same = lambda a, b: all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
    for flags in (256, 256 | 1, 256 | 4, 256 | 16, 256 | 64, 256 | 85):
        for k in (0, 3, 11):
            assert same(hip.parquet_read_column_host(zs, k, flags=flags), hip.parquet_read_column_host(plain.data, k))
    for k in (0, 3, 11):                                           # word 256 on an uncompressed file reads as flags 0
        assert same(hip.parquet_read_column_host(plain.data, k, flags=256), hip.parquet_read_column_host(plain.data, k))
    for flags, tail in REFUSAL_TAILS.items():                      # without 256 the refusal is what it was
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(zs, 0, flags=flags)
        assert e.value.code == EUNSUPPORTED and "ZSTD pages" in str(e.value) and str(e.value).endswith(tail)
    assert {p["codec"] for p in pages_of(zs, 0)} == {6}


def test_other_codecs_are_refused_with_the_flag_too(files):
    t = pa.table({"i": pa.array(np.arange(100, dtype=np.int32))})
    if pa.Codec.is_available("brotli"):
        br = C._write(files, "zs_refuse_brotli", t, compression="BROTLI").data
        for flags, text in ((ZSTD, "only UNCOMPRESSED and ZSTD pages are decoded"), (ZSTD | GZIP, "only UNCOMPRESSED, GZIP and ZSTD pages are decoded"),
                            (ZSTD | GZIP | SNAPPY | LZ4_RAW | DELTA, "only UNCOMPRESSED, SNAPPY, LZ4_RAW, GZIP and ZSTD pages are decoded")):
            with pytest.raises(hip.PlanHipError) as e:
                hip.parquet_read_column_host(br, 0, flags=flags)
            assert e.value.code == EUNSUPPORTED and "BROTLI pages" in str(e.value) and "(i)" in str(e.value) and str(e.value).endswith(text), str(e.value)
    for codec in ("SNAPPY", "LZ4_RAW", "GZIP"):
        data = C._write(files, "zs_refuse_" + codec.lower(), t, compression=codec).data
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(data, 0, flags=ZSTD)
        assert e.value.code == EUNSUPPORTED and codec + " pages" in str(e.value) and str(e.value).endswith("only UNCOMPRESSED and ZSTD pages are decoded")


def test_patches(files):
    for name, (orig, bad, column, page, word) in Z.patched(files, pages_of).items():
        good = hip.parquet_read_column_host(orig, column, flags=ZSTD)
        assert good[0] is not None
        with pytest.raises(hip.PlanHipError) as e:
            hip.parquet_read_column_host(bad, column, flags=ZSTD)
        msg = str(e.value)
        assert e.value.code == EINVAL and ("column %d (" % column) in msg and ("row group 0, page %d:" % page) in msg and word in msg, (name, msg)
        try:                                                       # the patch hit what it meant to: pyarrow raises or reads something else
            other = pq.read_table(pa.BufferReader(bad))
        except Exception:  # noqa: BLE001
            continue
        assert not other.equals(pq.read_table(pa.BufferReader(orig))), name
    both, column = Z.two_bad_pages(files, pages_of)
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(both, column, flags=ZSTD)
    assert e.value.code == EINVAL and "page 1: a corrupt ZSTD stream" in str(e.value)


SANITIZER_PROGRAM = r"""
#include "parquet_decode.h"
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

// argv: files. *.stream = an 8-byte little-endian expected length, then ONE ZSTD stream: decoded into a buffer of exactly that length
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
    const uint32_t flags = PH_PARQUET_ZSTD | PH_PARQUET_GZIP | PH_PARQUET_LZ4_RAW | PH_PARQUET_SNAPPY | PH_PARQUET_DELTA;
    for (int a = 1; a < argc; a++) {
        const std::string path = argv[a];
        std::vector<uint8_t> file = slurp(argv[a]);                 // exactly nbytes: one byte past the end is out of range
        if (path.size() > 7 && path.compare(path.size() - 7, 7, ".stream") == 0) {
            int64_t expected = 0;
            memcpy(&expected, file.data(), 8);
            if (expected > (1ll << 30)) { refused++; continue; }   // (what check_sizes refuses anyway: nothing is allocated for it)
            std::vector<uint8_t> stream(file.begin() + 8, file.end()), out((size_t)expected);
            if (ph::zstd::decompress_host(stream.data(), (int64_t)stream.size(), out.data(), expected) != ph::zstd::S_OK) refused++;
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
        pytest.fail("g++ not found: the sanitizer check of the ZSTD decoder needs a C++17 host compiler")
    src = tmp_path / "zstd_asan.cpp"
    src.write_text(SANITIZER_PROGRAM)
    exe = tmp_path / "zstd_asan"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                         f"-I{ROOT / 'plan_amd' / 'csrc'}", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    good = [(name, stream, len(out)) for name, stream, out in Z.valid_streams() + Z.pyarrow_streams()]
    bad = [c[:3] for c in Z.invalid_streams() + Z.stricter_streams()]
    paths = []
    for name, stream, n in good + bad:
        p = tmp_path / (name + ".stream")
        p.write_bytes(int(n).to_bytes(8, "little") + stream)
        paths.append(str(p))
    flagged = Z.flagged_files(files)
    paths += [c.path for c in cases.values()] + [c.path for c, _more in flagged.values()] + Z.write_patched(tmp_path, pages_of)
    both, _column = Z.two_bad_pages(files, pages_of)
    (tmp_path / "two_bad.parquet").write_bytes(both)
    paths.append(str(tmp_path / "two_bad.parquet"))
    ncols = sum(c.table.num_columns for c in cases.values()) + sum(c.table.num_columns for c, _more in flagged.values())
    run = subprocess.run([str(exe)] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    decoded, refused = (int(x) for x in run.stdout.split()[1::2])
    # (every patched file holds one column)
    assert decoded == len(good) + ncols and refused == len(bad) + len(Z.patched(files, pages_of)) + 1, run.stdout
