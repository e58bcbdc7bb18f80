"""The exploration noise's reference (tests/philox_ref.py) against Random123's published known answers for Philox4x32-10 - the reference the
GPU test of the in-kernel generator (test_gpu_actor_versions.py) compares krsel::normal4 with."""
import numpy as np
import pytest

from tests import philox_ref


@pytest.mark.parametrize("ctr,key,expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox4x32_10_reproduces_random123_known_answers(ctr, key, expect):
    got = tuple(int(x) for x in philox_ref.philox4x32_10(ctr, key))
    assert got == expect, [hex(x) for x in got]


def test_philox_vectorised_equals_scalar():
    rng = np.random.default_rng(0)
    c = [rng.integers(0, 2**32, 64, dtype=np.uint64) for _ in range(4)]
    k = [rng.integers(0, 2**32, 64, dtype=np.uint64) for _ in range(2)]
    vec = np.stack(philox_ref.philox4x32_10(c, k), 1)
    for i in range(64):
        assert tuple(vec[i]) == tuple(int(x) for x in philox_ref.philox4x32_10([x[i] for x in c], [x[i] for x in k]))


def test_normal4_reference_layout():
    """The counter words are (env, step low, step high, 0x4b52) and the key (seed low, seed high): a step or seed that differs only in its high word
    gives other draws, and the pairs (z0, z1), (z2, z3) share their radius."""
    z = philox_ref.normal4(0x1234_5678_9ABC_DEF0, 7, 3)
    assert z.shape == (4,) and np.isfinite(z).all()
    assert not np.array_equal(z, philox_ref.normal4(0x1234_5678_9ABC_DEF0, 7 + 2**32, 3))
    assert not np.array_equal(z, philox_ref.normal4(0x1234_5678_9ABC_DEF0 ^ (1 << 40), 7, 3))
    r = philox_ref.philox4x32_10((3, 7, 0, 0x4B52), (0x9ABCDEF0, 0x12345678))
    u0 = float(np.float32(int(r[0]) >> 8) + np.float32(0.5)) / 2**24
    assert np.hypot(z[0], z[1]) == pytest.approx(np.sqrt(-2 * np.log(u0)), rel=1e-12)
    zz = philox_ref.normal4(np.uint64(5), np.arange(20000, dtype=np.uint64), np.uint64(1)).ravel()
    assert abs(zz.mean()) < 0.02 and abs(zz.std() - 1) < 0.02
