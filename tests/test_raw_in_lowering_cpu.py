"""IN / NOT IN on raw INT / LONG / FLOAT / DOUBLE columns through the C++ planner (host.explain_filter: FilterPlanNode + FilterOperatorUtils as
text): the PG_PRED_RAW_SET leaf of Int / Long / Float / DoubleRawValueBasedInPredicateEvaluator (InPredicateEvaluatorFactory.java:74-107) --
its values as the int64 the ABI carries, sorted and de-duplicated; a FLOAT literal rounded once to float, then widened; the declines."""
import numpy as np
import pytest

from pinot_amd import _abi
from pinot_amd import host
from pinot_amd import query as Q
from test_oracle_range_not_queries import fp_edge_segment, range_segment

SELECT = "SELECT COUNT(*) FROM t WHERE "


@pytest.fixture(scope="module")
def segments():
    rs, fs = host.HostSegment(range_segment(), load=False), host.HostSegment(fp_edge_segment(3001)[0], load=False)
    yield rs, fs
    rs.destroy()
    fs.destroy()


def explain(seg, where):
    return host.explain_filter(seg, SELECT + where)


def test_the_leaf_of_every_raw_type(segments):
    rs, fs = segments
    assert explain(rs, "rawIntCol IN (500, -3, 250, 500, 2147483647, -2147483648)") == "SCAN(rawIntCol raw IN -2147483648,-3,250,500,2147483647)"
    assert explain(rs, "rawIntCol NOT IN (7)") == "SCAN(rawIntCol NOT raw IN 7)"
    assert explain(rs, "rawLongCol IN (9223372036854775807, -9223372036854775808, 5, 5)") == "SCAN(rawLongCol raw IN -9223372036854775808,5,9223372036854775807)"
    assert explain(rs, "rawLongCol NOT IN (4294967296, 1)") == "SCAN(rawLongCol NOT raw IN 1,4294967296)"
    # FLOAT: Float.parseFloat -- the literal is rounded ONCE, to float, and that float travels widened; DOUBLE: Double.parseDouble
    assert explain(fs, "f IN (0.1)") == "SCAN(f raw IN %d)" % Q.f64_bits(np.float32("0.1"))
    assert explain(fs, "d IN (0.1)") == "SCAN(d raw IN %d)" % Q.f64_bits(0.1)
    assert Q.f64_bits(np.float32("0.1")) != Q.f64_bits(0.1)
    assert explain(rs, "rawFloatCol IN (250.0, 2.5, 250)") == "SCAN(rawFloatCol raw IN %d,%d)" % (Q.f64_bits(2.5), Q.f64_bits(250.0))
    # (ascending as the int64 the ABI carries: negative doubles, sign bit set, come first)
    assert explain(rs, "rawDoubleCol NOT IN (1.5, -1.5)") == "SCAN(rawDoubleCol NOT raw IN %d,%d)" % (Q.f64_bits(-1.5), Q.f64_bits(1.5))
    assert explain(fs, "d IN (1e400)") == "SCAN(d raw IN %d)" % Q.f64_bits(np.inf)      # Double.parseDouble overflows to Infinity


def test_inside_and_or_not(segments):
    rs, _ = segments
    # two scan leaves keep the query's order (equal priority, stable sort)
    assert explain(rs, "rawIntCol IN (3, 4) AND dictionarizedIntCol > 5") == "AND(SCAN(rawIntCol raw IN 3,4), SCAN(dictionarizedIntCol dictIds 1..999))"
    assert explain(rs, "dictionarizedIntCol > 5 AND rawLongCol NOT IN (3)") == "AND(SCAN(dictionarizedIntCol dictIds 1..999), SCAN(rawLongCol NOT raw IN 3))"
    assert explain(rs, "rawIntCol IN (3) OR rawDoubleCol IN (2.5)") == "OR(SCAN(rawIntCol raw IN 3), SCAN(rawDoubleCol raw IN %d))" % Q.f64_bits(2.5)
    assert explain(rs, "NOT (rawIntCol IN (3) OR rawLongCol IN (4))") == "NOT(OR(SCAN(rawIntCol raw IN 3), SCAN(rawLongCol raw IN 4)))"
    assert explain(rs, "rawIntCol BETWEEN 1 AND 9 AND NOT rawIntCol IN (5)") == "AND(SCAN(rawIntCol raw 1..9), NOT(SCAN(rawIntCol raw IN 5)))"


def test_declines(segments):
    rs, fs = segments
    for where in ("rawIntCol IN (5, 2147483648)", "rawIntCol IN (1.5)", "rawLongCol NOT IN (9223372036854775808)", "rawFloatCol IN (abc)"):
        with pytest.raises(host.HostError) as e:
            explain(rs, where)
        assert e.value.status == 1, where
    with pytest.raises(host.HostError, match="Cannot convert value") as e:
        explain(rs, "rawIntCol IN (5, 2147483648)")
    for seg, where in ((rs, "rawFloatCol IN (1.5, 0.0)"), (rs, "rawDoubleCol NOT IN (-0.0)"), (rs, "rawDoubleCol IN (0)"), (fs, "f IN (1e-60)"), (fs, "d IN ('NaN', 1.0)"),
                       (fs, "f NOT IN ('NaN')")):
        with pytest.raises(host.HostError) as e:
            explain(seg, where)
        assert e.value.status == 2, where
    cap = _abi.PG_RAW_SET_MAX_VALUES
    assert explain(rs, "rawIntCol IN (%s)" % ", ".join(str(v) for v in range(cap))).count(",") == cap - 1
    assert explain(rs, "rawIntCol IN (%s)" % ", ".join(str(v % cap) for v in range(3 * cap))).count(",") == cap - 1      # the cap counts distinct values
    for column in ("rawIntCol", "rawLongCol", "rawFloatCol", "rawDoubleCol"):
        with pytest.raises(host.HostError) as e:
            explain(rs, "%s NOT IN (%s)" % (column, ", ".join(str(v + 1) for v in range(cap + 1))))
        assert e.value.status == 2, column


def test_a_dictionary_column_is_lowered_as_before(segments):
    rs, _ = segments
    assert explain(rs, "dictionarizedIntCol IN (500, 600, 7)") == "SCAN(dictionarizedIntCol in 2 dictIds)"
    assert explain(rs, "dictionarizedIntCol NOT IN (500)") == "SCAN(dictionarizedIntCol NOT in 1 dictIds)"
    assert explain(rs, "rawIntCol BETWEEN 250 AND 500") == "SCAN(rawIntCol raw 250..500)"
    assert explain(rs, "rawIntCol = 5") == "SCAN(rawIntCol raw 5..5)"
