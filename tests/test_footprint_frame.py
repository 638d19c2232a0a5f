"""The footprint frame (tests/footprint.py) reports what it is there to report: numpy stands in for the device, a few lines of
Python for the kernel.  Each stray write must come back under the right name and offset, and a clean call must report nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402

N, ZONE = 64, 128


@pytest.fixture
def frame():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 40, size=(3, 2, 1, N), dtype=np.uint64)
    b = rng.integers(0, 1 << 40, size=(3, 2, 1, N), dtype=np.uint64)
    f = fp.Frame(fp.HostDevice(), [("a", a), ("b", b), ("out", a.size)], ZONE)
    f.a, f.b = a, b
    yield f
    f.close()


def _add(frame, first=0, words=None, at=0):
    """the 'kernel': out[at + i] = a[i] + b[i] for i in first .. first + words - 1"""
    words = frame.a.size - first if words is None else words
    out = fp.HostDevice.words_at(frame.ptr("out"), frame.a.size + ZONE)  # the zone behind it included: an overrun lands there
    out[at + first:at + first + words] = (frame.a.reshape(-1) + frame.b.reshape(-1))[first:first + words]


def test_layout_is_aligned_and_zoned(frame):
    assert frame.order == ["a", "b", "out"] and set(frame.zones) == {"zone0", "zone1", "zone2", "zone3"}
    for name in frame.order:
        assert frame.ptr(name).value % 16 == 0 and frame.offset(name) % 2 == 0
        assert frame.zones[frame.zone_before(name)][1] >= ZONE
    assert frame.zones["zone3"][1] >= ZONE
    covered = sorted(list(frame.zones.values()) + list(frame.parts.values()))
    assert covered[0][0] == 0 and all(o + w == covered[i + 1][0] for i, (o, w) in enumerate(covered[:-1]))
    assert covered[-1][0] + covered[-1][1] == frame.words
    assert int(frame.initial[5]) == fp.SENTINEL ^ 5 and int(fp.SENTINEL) >> 63 == 1


def test_odd_part_keeps_the_next_part_aligned():
    f = fp.Frame(fp.HostDevice(), [("x", np.arange(7, dtype=np.uint64)), ("y", 3)], 9)
    assert f.offset("x") % 2 == 0 and f.offset("y") % 2 == 0
    assert f.zones[f.zone_after("x")] == (f.offset("x") + 7, f.offset("y") - f.offset("x") - 7) and f.zones["zone1"][1] >= 10
    fp.HostDevice.words_at(f.ptr("x"), 8)[7] = 1  # the pad word behind an odd part belongs to the zone behind it
    assert f.check().changed == {"zone1": (1, 0)}


def test_clean_call_reports_nothing(frame):
    _add(frame)
    res = frame.check(written={"out"})
    assert res.clean and res.changed == {} and res.unwritten == {}
    assert np.array_equal(res.part("out", frame.a.shape), frame.a + frame.b)


def test_untouched_frame_reports_the_unwritten_output(frame):
    res = frame.check(written={"out"})
    assert res.changed == {} and res.unwritten == {"out": (frame.a.size, 0)}


def test_one_word_past_the_output(frame):
    _add(frame, words=frame.a.size)
    fp.HostDevice.words_at(frame.ptr("out", frame.a.size), 1)[0] = 12345
    res = frame.check(written={"out"})
    assert res.changed == {frame.zone_after("out"): (1, 0)} and res.unwritten == {}


def test_one_word_in_front_of_the_output(frame):
    _add(frame)
    fp.HostDevice.words_at(frame.ptr("out", -1), 1)[0] = 12345
    res = frame.check(written={"out"})
    last = frame.zones[frame.zone_before("out")][1] - 1
    assert res.changed == {frame.zone_before("out"): (1, last)} and frame.zone_before("out") == frame.zone_after("b")


def test_one_output_word_left_unwritten(frame):
    _add(frame, words=100)
    _add(frame, first=101)
    res = frame.check(written={"out"})
    assert res.changed == {} and res.unwritten == {"out": (1, 100)} and not res.clean


def test_one_operand_word_changed(frame):
    _add(frame)
    fp.HostDevice.words_at(frame.ptr("b"), frame.b.size)[17] ^= np.uint64(1)
    res = frame.check(written={"out"})
    assert res.changed == {"b": (1, 17)} and res.unwritten == {}


def test_displaced_output_is_seen_on_both_sides(frame):
    """a whole result stored two words late: two sentinels survive at the front, two zone words change behind"""
    _add(frame, at=2)
    res = frame.check(written={"out"})
    assert res.unwritten == {"out": (2, 0)} and res.changed == {frame.zone_after("out"): (2, 0)}


def test_displaced_sentinel_is_seen(frame):
    """a copy of a neighbouring zone word is not the word that belongs there"""
    _add(frame)
    zone = fp.HostDevice.words_at(frame.ptr("out", frame.a.size), 4)
    zone[1] = zone[0]
    assert frame.check(written={"out"}).changed == {frame.zone_after("out"): (1, 1)}


def test_in_place_part_is_returned_not_reported(frame):
    """out aliased to operand a: a is written, b and the zones must stay"""
    fp.HostDevice.words_at(frame.ptr("a"), frame.a.size)[:] = (frame.a + frame.b).reshape(-1)
    res = frame.check(written={"a"})
    assert res.changed == {} and res.unwritten == {}
    assert np.array_equal(res.part("a", frame.a.shape), frame.a + frame.b)
    assert set(frame.check(written=()).changed) == {"a"}  # the same image, nothing declared written


def test_doubles_and_counts_are_parts():
    re = np.linspace(-1.0, 1.0, 8)
    f = fp.Frame(fp.HostDevice(), [("re", re), ("out", np.int64(4))], 2)
    assert np.array_equal(f.check().part("re", dtype=np.float64), re) and "out" in f.prefilled
    with pytest.raises(ValueError):
        fp.Frame(fp.HostDevice(), [("bytes", np.zeros(8, dtype=np.int8))], 2)
    with pytest.raises(ValueError):
        fp.Frame(fp.HostDevice(), [("x", 2), ("x", 2)], 2)


def test_zone_words_for():
    assert fp.zone_words_for(64, (3, 2, 1, 64)) == 128 and fp.zone_words_for(64, (3, 3, 2, 64), (3, 2, 2, 64)) == 384
    assert fp.zone_words_for(4096, (1, 4096)) == 8192
