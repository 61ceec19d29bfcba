"""tests/dev/devcheck.hip built as a plain host program (-DDEVCHECK_HOST:
kernels replaced by loops): the lane field layer, the scalars and the hashes
over the case sets of tests/dev/devcases.py, against the same Python-integer
references the GPU tests use. No GPU needed -- this is what shows the case
generators and references right; tests/test_device_primitives_gpu.py then
runs the same checks on the device lowering."""
import os

import pytest

from tests.dev import devcases
from tests.host import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dev", "devcheck.hip")
BIN = os.path.join(ROOT, "build", "devcheck_host")


@pytest.fixture(scope="module")
def run():
    return devcases.runner(hostbuild.build(SRC, BIN, ["-std=c++20", "-x", "c++", "-DDEVCHECK_HOST"]))


def test_product_excess_is_tiny():
    """what the product checks allow limbs 1 and 5 above 2^25 - 1 (derived in
    devcases.reduce64_excess from fe_reduce64 at MUL_BOUND inputs): "tiny", so
    sums of a few products stay far inside MUL_BOUND"""
    assert set(devcases.PRODUCT_EXCESS) == {1, 5}
    assert all(0 < e < 2**13 for e in devcases.PRODUCT_EXCESS.values()), devcases.PRODUCT_EXCESS


@pytest.mark.parametrize("name", list(devcases.LANE_CHECKS))
def test_lane_primitive_host(run, name):
    devcases.LANE_CHECKS[name](run)
