"""rt_gather_rows and rt_gather_max_rows (include/rt_gather.h, librtgather.so): the host
arithmetic of the cyclic row deal, against a brute-force count. The library loads without a
device (its kernels and RCCL are only reached through the other entry points)."""
import pytest

from surely_rt.parallel import cyclic_rows, gather_lib, max_rows


@pytest.fixture(scope="module")
def lib():
    return gather_lib()


def test_rows_and_max_rows_against_a_count(lib):
    for height in range(0, 41):
        for world in range(1, 10):
            rows = [lib.rt_gather_rows(height, world, r) for r in range(world)]
            count = [sum(1 for y in range(height) if y % world == r) for r in range(world)]
            assert rows == count, (height, world)
            assert sum(rows) == height
            assert lib.rt_gather_max_rows(height, world) == rows[0] == max(rows)
            # the Python mirror bench.py deals rows with
            assert [cyclic_rows(height, r, world)[2] for r in range(world)] == rows
            assert max_rows(height, world) == rows[0]


def test_bad_arguments_give_zero(lib):
    assert lib.rt_gather_rows(-1, 3, 0) == 0
    assert lib.rt_gather_rows(7, 0, 0) == 0
    assert lib.rt_gather_rows(7, -2, 0) == 0
    assert lib.rt_gather_rows(7, 3, -1) == 0
    assert lib.rt_gather_rows(7, 3, 3) == 0  # rank >= world
    assert lib.rt_gather_max_rows(0, 3) == 0
    assert lib.rt_gather_max_rows(-5, 3) == 0
    assert lib.rt_gather_max_rows(7, 0) == 0
    assert lib.rt_gather_max_rows(7, -1) == 0
    # no overflow in (height - rank + world - 1) near INT_MAX / 2
    assert lib.rt_gather_rows(2**30, 2**30, 2**30 - 1) == 1
