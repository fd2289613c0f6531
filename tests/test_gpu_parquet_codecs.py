"""The error word across the three section launches of one load. tests/codec_order_cases.py patches one page's stream in a SNAPPY, an
LZ4_RAW and a GZIP column of one file, so that each launch of ph_table_create_parquet_ex finds a corrupt section of its own; the load
must refuse with exactly what the file with only the lowest (column, page) patched gives — whichever codec, and so whichever launch, owns
that page — and the unpatched file loads on the same context afterwards. tests/test_codec_order_reference.py pins the host twin's
message for each of these pages."""
import pytest

import codec_order_cases as C
from parquet_codec_helpers import load_and_compare
from plan_amd import hip, loader

pytestmark = pytest.mark.gpu

ALL = hip.PH_PARQUET_SNAPPY | hip.PH_PARQUET_LZ4_RAW | hip.PH_PARQUET_GZIP


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("codec_order")


def pages_of(data, column):
    return loader.parquet_pages(data, column, codecs=True)


def refusal(f, *a, **kw):
    with pytest.raises(hip.PlanHipError) as e:
        f(*a, **kw)
    return e.value.code, str(e.value)


@pytest.mark.parametrize("name", sorted(C.ARRANGEMENTS))
def test_three_corrupt_codecs_name_the_lowest_page(ctx, files, name):
    case, arrangements = C.arrangements(files, pages_of)
    all3, singles = arrangements[name]
    column, page, row_group, codec, lowest_alone = singles[0]
    code, msg = refusal(loader.table_from_parquet_device, ctx, all3, flags=ALL)
    assert (code, msg) == refusal(loader.table_from_parquet_device, ctx, lowest_alone, flags=ALL)
    tail = "column %d (%s): row group %d, page %d: a corrupt %s stream" % (column, case.table.column_names[column], row_group, page, codec)
    assert code == hip.PH_EINVAL and msg.split(": ", 2)[2] == tail, msg
    hcode, hmsg = refusal(hip.parquet_read_column_host, all3, column, flags=ALL)
    assert hcode == code and hmsg.split(": ", 2)[2] == tail      # the host twin says the same behind its own name
    for other in singles[1:]:                                    # each of the other two is refused alone, with its own page
        ocode, omsg = refusal(loader.table_from_parquet_device, ctx, other[4], flags=ALL)
        assert ocode == hip.PH_EINVAL and omsg.endswith(": row group %d, page %d: a corrupt %s stream" % (other[2], other[1], other[3])), omsg
    load_and_compare(ctx, case, ALL, files)                      # the unpatched file loads, on the same context
