"""The cases of tests/codec_order_cases.py on the host, no device: one file with a corrupt page in a SNAPPY, an LZ4_RAW and a GZIP column.
ph_parquet_read_column_host reads one column at a time, so it names each column's own page: the same message for a page whether the
other two are patched or not, behind checks that all pass (only the decoder refuses). tests/test_gpu_parquet_codecs.py holds the device
load, which decodes all columns in one call and must name the lowest, to these messages."""
import pytest

import codec_order_cases as C
from plan_amd import hip, loader

ALL = hip.PH_PARQUET_SNAPPY | hip.PH_PARQUET_LZ4_RAW | hip.PH_PARQUET_GZIP


def pages_of(data, column):
    return loader.parquet_pages(data, column, codecs=True)


def host_message(data, column):
    with pytest.raises(hip.PlanHipError) as e:
        hip.parquet_read_column_host(data, column, flags=ALL)
    assert e.value.code == hip.PH_EINVAL
    return str(e.value).split(": ", 2)[2]                        # behind the function's name and the code


@pytest.mark.parametrize("name", sorted(C.ARRANGEMENTS))
def test_each_patched_column_names_its_own_page_whatever_else_is_patched(tmp_path_factory, name):
    case, arrangements = C.arrangements(tmp_path_factory.mktemp("codec_order"), pages_of)
    all3, singles = arrangements[name]
    patched_columns = [s[0] for s in singles]
    for column, page, row_group, codec, alone in singles:
        want = "column %d (%s): row group %d, page %d: a corrupt %s stream" % (column, case.table.column_names[column], row_group, page, codec)
        assert host_message(all3, column) == host_message(alone, column) == want
        for other in patched_columns:                            # the patch touches this column's page alone
            if other != column:
                hip.parquet_read_column_host(alone, other, flags=ALL)
    for column in range(case.table.num_columns):                # and every other column of the patched file reads as the original's
        if column not in patched_columns:
            got, want = hip.parquet_read_column_host(all3, column, flags=ALL), hip.parquet_read_column_host(case.data, column, flags=ALL)
            assert [None if a is None else bytes(a) for a in got] == [None if b is None else bytes(b) for b in want], column
