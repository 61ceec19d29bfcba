"""The pipelined window sums of k_verify_quad_hs_fold on the host
(tests/host/sumpipecheck.cpp): quad.h h_window_addend_front / _back, the two
halves a wave forms its window's S_w = [dA](-A) + [dR](-/+R) from in two
successive windows, and h_sums_pipe, the loop the hash helper and the comb
wave both run -- here by two host threads that meet only at the window
barriers, as on the device.

The stand-alone program is built three ways, as tests/test_sum_split_host.py
builds sumsplitcheck: plain, with the operand bound assertions
(-DCMTV_BOUNDS_CHECK), and with AddressSanitizer + UBSan.

 - halves: tables of (0..8)P for random points, the identity, points of order
   8, 4 and 2 and rescaled ones (Z != 1); every dA, dR in -8..8 and both r_flip
   (so both signs of either operand): front + back is h_window_addend limb for
   limb.
 - schedule: every W from 2 to HS_MAX_WINDOWS and HS_WIDE_WINDOWS: every read
   of a ring slot finds its own window's sum, no slot is rewritten before it
   was read, each wave meets W - 1 barriers, the owners alternate from the
   lead at W - 2 (so the last window's owner differs between odd and even W).
 - fold: q_verify_hs_fold in foldcheck.cpp's four-lane-thread harness with S_w
   from the two waves' threads, over the corpus and the 35- / 36-window
   vectors, window counts raised by 0..2, and on the forced 64-window
   fallback; every verdict against the undivided sums' and the oracle's
   committed one.
No GPU needed."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.host import hostbuild

from test_host_math import _keyed_subset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "sumpipecheck.cpp")

BUILDS = {
    "plain": ["-std=c++20", "-pthread"],
    "bounds": ["-std=c++20", "-pthread", "-DCMTV_BOUNDS_CHECK"],
    "asan_ubsan": ["-std=c++20", "-pthread", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}
# 14 tables, 3 partners each, 17 x 17 digit pairs, 2 flips
HALF_CASES = 14 * 3 * 17 * 17 * 2
# W = 2 .. HS_MAX_WINDOWS (37) and HS_WIDE_WINDOWS
SCHEDULES = 36 + 1


@pytest.fixture(scope="module", params=list(BUILDS))
def binary(request):
    kind = request.param
    return hostbuild.build(SRC, os.path.join(ROOT, "build", f"sumpipecheck_{kind}"), BUILDS[kind]), kind


def test_halves_reproduce_the_whole_sum_limb_for_limb(binary):
    r = subprocess.run([binary[0], "halves"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip() == f"ok {HALF_CASES} cases", r.stdout


def test_schedule_for_every_window_count(binary):
    r = subprocess.run([binary[0], "schedule"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip() == f"ok {SCHEDULES} schedules", r.stdout


def _run(binary, args, pk, sig, msgs, mode):
    buf = [struct.pack("<I", len(msgs))]
    for p, s, m in zip(pk, sig, msgs):
        buf.append(bytes([mode]) + bytes(p) + bytes(s) + struct.pack("<I", len(m)) + m)
    r = subprocess.run([binary] + args, input=b"".join(buf), capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.frombuffer(r.stdout, np.uint8).reshape(-1, 2)
    assert len(got) == len(msgs)
    return got[:, 0], got[:, 1]


def _check(pipe, whole, want, names):
    bad = np.nonzero((pipe != want) | (whole != want))[0]
    assert bad.size == 0, [(names[int(i)], int(pipe[i]), int(whole[i]), int(want[i])) for i in bad[:10]]


@pytest.mark.parametrize("mode,key", [(0, "go"), (1, "zip215")])
@pytest.mark.parametrize("args", [["fold"], ["fold", "wide"]], ids="-".join)
def test_pipelined_sums_match_undivided_and_oracle_on_corpus(binary, corpus, mode, key, args):
    """Every adversarial vector class and a slice of the honest ones; the
    forced-wide runs take a thinner slice."""
    step = 5 if len(args) == 1 else 13
    idx = _keyed_subset(corpus)[mode::step]
    cats = [corpus["cats"][i] for i in idx]
    assert len(set(cats)) >= 4
    pipe, whole = _run(binary[0], args, corpus["pk"][idx], corpus["sig"][idx], [corpus["msgs"][i] for i in idx], mode)
    _check(pipe, whole, corpus[key][idx], list(zip(idx, cats)))


@pytest.mark.parametrize("mode,key", [(0, "go"), (1, "zip215")])
def test_pipelined_sums_on_wide_vectors(binary, mode, key):
    """The 35- and 36-window pairs (raised by up to 2 more by position): odd and
    even window counts, so either wave stores the last sum."""
    with open(os.path.join(ROOT, "tests", "golden", "wide_vectors.json")) as f:
        wide = json.load(f)["ed25519"]
    want = np.array([v[key] for v in wide], np.uint8)
    assert {35, 36} <= {v["windows"] for v in wide}
    pipe, whole = _run(binary[0], ["fold"], [bytes.fromhex(v["pk"]) for v in wide],
                       [bytes.fromhex(v["sig"]) for v in wide], [bytes.fromhex(v["msg"]) for v in wide], mode)
    _check(pipe, whole, want, [v["cat"] for v in wide])
