"""One file, three corrupt pages, one in each codec: the cases of tests/test_codec_order_reference.py (host twin) and
tests/test_gpu_parquet_codecs.py (device). The device load decompresses the SNAPPY, LZ4_RAW and GZIP sections of a call in three launches
that share one error word; whichever launch finds its page corrupt, the load must name the lowest (column, page) of the call.

The file is gzip_cases.flagged_files' mixed_codecs (row groups of 1100 rows, every column in a codec of its own). Its v2 data pages are
stored uncompressed (they do not shrink), so the compressed pages are the dictionary pages: one per column and row group, pages 0, 2 and 4
of the column's directory. Every patch leaves what the host checks before decoding alone (the sizes, Snappy's preamble, the GZIP header):
only the decoder can refuse it."""
import gzip_cases as G
import lz4_cases as L4
import snappy_cases as SN

SNAPPY, LZ4_RAW, GZIP = 1, 7, 2            # parquet.thrift's CompressionCodec
NAMES = {SNAPPY: "SNAPPY", LZ4_RAW: "LZ4_RAW", GZIP: "GZIP"}

# (column, page) per codec; the first entry is the lowest column and takes a LATER page than the others, so that a load that orders the
# pages by anything but (column, page) names another one. Columns of mixed_codecs: 0, 7, 11 SNAPPY; 3, 6, 9 LZ4_RAW; 1, 4, 8, 10, 13 GZIP.
ARRANGEMENTS = {
    "snappy_lowest": [(0, 4), (1, 0), (3, 2)],
    "gzip_lowest": [(1, 2), (3, 0), (11, 0)],          # (11: a BYTE_ARRAY dictionary, judged in front of its column's data pages)
    "lz4_lowest": [(3, 4), (4, 2), (7, 0)],
}


def corrupt_stream(codec, stream):
    """(position in the stream, new bytes): a patch that the codec's decoder must refuse whatever the stream holds"""
    if codec == GZIP:
        return len(stream) - 7, bytes([stream[-7] ^ 0x40])                    # a bit of the member's CRC-32
    if codec == LZ4_RAW:
        seqs = L4.sequences(stream)
        with_match = [s for s in seqs if s[3] is not None]
        if with_match:
            return with_match[0][3], b"\0\0"                                  # offset 0
        tpos, ln, lpos, _opos, _off, _mlen = seqs[-1]                         # literals only: one more (or one fewer) than the block holds
        assert ln >= 15 and lpos - 1 > tpos, seqs[-1]
        b = stream[lpos - 1]
        return lpos - 1, bytes([b + 1 if b < 254 else b - 1])
    assert codec == SNAPPY
    els = SN.elements(stream)
    far = [e for e in els if e[1] == 2]
    if far:
        return far[0][0] + 1, b"\0\0"                                        # a copy with a two-byte offset: offset 0
    pos, kind, n, _first = els[-1]                                            # literals only: the last one a byte longer than its input
    assert kind == 0
    if n <= 59:
        return pos, bytes([stream[pos] + 4])
    assert stream[pos + 1] != 0xff
    return pos + 1, bytes([stream[pos + 1] + 1])


def arrangements(dirpath, pages_of):
    """(the unpatched Case, {name: (all three patched, [(column, page, row group, codec name, that page alone patched)] lowest first)})"""
    case, _more = G.flagged_files(dirpath)["mixed_codecs"]
    data = case.data
    out = {}
    for name, where in ARRANGEMENTS.items():
        assert where == sorted(where) and len(where) == 3
        all3, singles = bytearray(data), []
        for column, page in where:
            p = pages_of(data, column)[page]
            assert p["compressed"] == 1 and p["data_bytes"] > 0, (name, column, page)
            stream = data[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
            at, new = corrupt_stream(p["codec"], stream)
            assert stream[at:at + len(new)] != new, (name, column, page)
            at += p["data_pos"]
            all3[at:at + len(new)] = new
            singles.append((column, page, p["row_group"], NAMES[p["codec"]], data[:at] + new + data[at + len(new):]))
        assert sorted(s[3] for s in singles) == ["GZIP", "LZ4_RAW", "SNAPPY"], name
        out[name] = (bytes(all3), singles)
    assert sorted(s[0][3] for _b, s in out.values()) == ["GZIP", "LZ4_RAW", "SNAPPY"]     # each codec owns the lowest page once
    return case, out
