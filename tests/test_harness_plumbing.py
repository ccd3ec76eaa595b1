"""tests/harness.py itself: the reader of result files and the bit-for-bit comparison every host harness and GPU comparison goes
through.  No program is built or run."""
import struct

import numpy as np
import pytest

import harness


def test_reader_round_trip_over_mixed_dtypes(tmp_path):
    f32 = np.array([[1.5, -0.0, np.nan], [np.inf, 2.0 ** -149, -3.25]], np.float32)
    u8, i64, u64 = np.array([0, 255, 7], np.uint8), np.array([-2 ** 63, 2 ** 63 - 1], np.int64), np.array([2 ** 64 - 1], np.uint64)
    path = tmp_path / "blob.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<iIQ", -5, 0xFFFFFFFF, 2 ** 40))
        harness.put(f, (f32, np.float32), (u8, np.uint8), (i64.tolist(), np.int64), (u64, np.uint64), ([], np.float32))
    r = harness.Reader.of_file(path)
    assert r.unpack("<iIQ") == (-5, 0xFFFFFFFF, 2 ** 40)
    got = r.take(6, np.float32, (2, 3))
    assert got.shape == (2, 3) and got.dtype == np.float32 and got.tobytes() == f32.tobytes()
    assert np.array_equal(r.take(3, np.uint8), u8) and np.array_equal(r.take(2, np.int64), i64) and np.array_equal(r.take(1, np.uint64), u64)
    assert r.take(0, np.float32).size == 0
    r.done()
    got[0, 0] = 9.0                                              # a copy: the blob stays as it was read
    assert harness.Reader.of_file(path).unpack("<iIQf")[3] == 1.5


def test_done_fails_on_a_leftover_byte():
    r = harness.Reader(np.arange(3, dtype=np.uint32).tobytes() + b"\x00")
    r.take(3, np.uint32)
    with pytest.raises(AssertionError, match="1 bytes"):
        r.done()


def test_take_and_unpack_past_the_end_fail():
    r = harness.Reader(bytes(10))
    r.take(2, np.float32)
    with pytest.raises(AssertionError):
        r.take(1, np.float32)                                    # two bytes are left
    with pytest.raises(AssertionError):
        r.unpack("<I")
    assert r.take(2, np.uint8).size == 2                         # neither failure consumed anything
    r.done()


def test_assert_same_bits_sees_the_sign_of_zero_one_bit_of_a_byte_and_a_shape():
    base = dict(dist2=np.zeros(5, np.float32), feature=np.full(5, 3, np.uint8), point=np.ones((5, 3), np.float32))
    same = {k: v.copy() for k, v in base.items()}
    harness.assert_same_bits(same, base, "equal", tuple(base))
    harness.assert_same_bits(dict(same, dist2=same["dist2"].view(np.int32)), base, "equal item size", tuple(base))

    minus_zero = dict(same, dist2=np.array([0, 0, -0.0, 0, 0], np.float32))
    assert np.array_equal(minus_zero["dist2"], base["dist2"])    # equal as values
    with pytest.raises(AssertionError, match="dist2 differs on 1 of 5 rows, first 2"):
        harness.assert_same_bits(minus_zero, base, "-0", tuple(base))
    harness.assert_same_bits(minus_zero, base, "-0", ("feature", "point"))         # only the named fields are compared

    one_bit = dict(same, feature=np.array([3, 3, 3, 3, 2], np.uint8))
    with pytest.raises(AssertionError, match="feature differs on 1 of 5 rows, first 4"):
        harness.assert_same_bits(one_bit, base, "bit", tuple(base))

    for other in (np.ones((5, 1, 3), np.float32), np.ones(15, np.float32), np.ones((4, 3), np.float32), np.ones((5, 3), np.float64)):
        with pytest.raises(AssertionError):
            harness.assert_same_bits(dict(same, point=other), base, "shape", tuple(base))


def test_to_numpy_views_the_named_fields_and_passes_the_rest_through():
    counters = object()
    res = harness.to_numpy(dict(vertex0=np.array([-1, 6], np.int32), group=np.array([-1, 0], np.int32), counters=counters), ("vertex0",))
    assert res["vertex0"].dtype == np.uint32 and res["vertex0"].tolist() == [0xFFFFFFFF, 6]
    assert res["group"].dtype == np.int32 and res["counters"] is counters
