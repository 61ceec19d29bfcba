"""fe_mul / fe_sq / fe_sqn in both carry chains (fe25519.h: the serial chain,
whose carries ride the next column's first multiply-add, and the ref10 chain
of fe_reduce64) against 256-bit integer arithmetic mod 2^255 - 19, on the
host: tests/host/fecheck.cpp, a stand-alone program, built once with the
header's bounds assertions on (operands, "column sum plus incoming carry
< 2^64", output limbs) and once with AddressSanitizer + UBSan.

Cases: every limb at MUL_BOUND - 1; odd limbs at SQ_ODD_BOUND - 1; zero, p,
2p, p - 1 (limb-wise); 10^5 random lazy inputs. Every result is compared
with the integer product, every output limb with the carried bounds, and
the two chains with each other as field elements."""
import os
import subprocess

import pytest

from tests.host import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "fecheck.cpp")

BUILDS = {
    "bounds": ["-std=c++17", "-DCMTV_BOUNDS_CHECK"],
    "asan_ubsan": ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("kind", list(BUILDS))
def test_fe_products_match_integers(kind):
    binary = hostbuild.build(SRC, os.path.join(ROOT, "build", f"fecheck_{kind}"), BUILDS[kind])
    r = subprocess.run([binary, "100000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok 100036 cases"), r.stdout


def test_serial_chain_limb1_excess():
    """the excess of limb 1 that fecheck allows (2^13), from the largest column
    sums: the serial chain on every limb of both operands at MUL_BOUND - 1,
    every column below 2^64 with its carry"""
    b = 226000000 - 1
    h = [0] * 10
    for i in range(10):
        for j in range(10):
            h[(i + j) % 10] += (2 if i & 1 and j & 1 else 1) * (19 if i + j >= 10 else 1) * b * b
    for i in range(9):
        h[i + 1] += h[i] >> (25 if i & 1 else 26)
        assert h[i + 1] < 2**64
    excess = ((2**26 - 1) + 19 * (h[9] >> 25)) >> 26
    assert 0 < excess < 2**13, excess
    # what the device checks of tests/dev/devcases.py allow on limb 1
    from tests.dev import devcases
    assert excess <= devcases.PRODUCT_EXCESS[1], (excess, devcases.PRODUCT_EXCESS)
