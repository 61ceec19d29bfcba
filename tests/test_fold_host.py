"""The folded helper-summed quad verifier (quad.h q_verify_hs_fold, the source
of k_verify_quad_hs_fold) compiled for the host with the operand bound
assertions on (tests/host/foldcheck.cpp): X = [k1](-A) + [k2](P_s - R) with
P_s = [s]B from the 16-position comb on s, no fixed-base digit in any window.
Four threads run the quad in lockstep; the comb wave's share of P_s (its top
0..16 positions, by vector; the quad adds the rest), the helper's scalars
(without u) and its window sums are computed as those waves do.

Every vector's verdict must equal q_verify_hs's (the form it replaces, run in
the same program on the same window count) and the oracle's committed one,
with the window count raised by 0..2, on the 64-window fallback, and with the
quads adding every comb row themselves (the path of a wave that stopped
waiting for the comb wave). No GPU needed."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import coracle
from tests.host import hostbuild

from test_host_math import _keyed_subset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FSRC = os.path.join(ROOT, "tests", "host", "foldcheck.cpp")
FBIN = os.path.join(ROOT, "build", "foldcheck")
L = 2**252 + 27742317777372353535851937790883648493


@pytest.fixture(scope="module")
def foldcheck():
    return hostbuild.build(FSRC, FBIN, ["-std=c++20", "-pthread"])


@pytest.fixture(scope="module")
def wide_ed():
    with open(os.path.join(ROOT, "tests", "golden", "wide_vectors.json")) as f:
        return json.load(f)["ed25519"]


def _run(binary, args, pk, sig, msgs, mode):
    buf = [struct.pack("<I", len(msgs))]
    for p, s, m in zip(pk, sig, msgs):
        buf.append(bytes([mode]) + bytes(p) + bytes(s) + struct.pack("<I", len(m)) + m)
    out = subprocess.run([binary] + args, input=b"".join(buf), capture_output=True, check=True, timeout=600).stdout
    got = np.frombuffer(out, np.uint8).reshape(-1, 2)
    assert len(got) == len(msgs)
    return got[:, 0], got[:, 1]


def _check(fold, hs, want, names):
    bad = np.nonzero((fold != want) | (hs != want))[0]
    assert bad.size == 0, [(names[int(i)], int(fold[i]), int(hs[i]), int(want[i])) for i in bad[:10]]


@pytest.mark.parametrize("mode,key", [(0, "go"), (1, "zip215")])
@pytest.mark.parametrize("args", [["fold"], ["late"], ["fold", "wide"], ["late", "wide"]], ids="-".join)
def test_fold_matches_hs_and_oracle_on_corpus(foldcheck, corpus, mode, key, args):
    """Every adversarial vector class (small and mixed order, non-canonical
    encodings, s >= L) and a slice of the honest ones. The forced-wide and
    late runs take thinner slices at other offsets."""
    step = {"fold": 4, "late": 9, "fold-wide": 11, "late-wide": 17}["-".join(args)]
    idx = _keyed_subset(corpus)[len(args) % 2::step]
    cats = [corpus["cats"][i] for i in idx]
    assert len(set(cats)) >= 4
    fold, hs = _run(foldcheck, args, corpus["pk"][idx], corpus["sig"][idx], [corpus["msgs"][i] for i in idx], mode)
    _check(fold, hs, corpus[key][idx], list(zip(idx, cats)))


@pytest.mark.parametrize("mode,key", [(0, "go"), (1, "zip215")])
@pytest.mark.parametrize("args", [["fold"], ["late"]], ids="-".join)
def test_fold_on_wide_vectors(foldcheck, wide_ed, mode, key, args):
    """The 35- and 36-window pairs (raised by up to 2 more by position)."""
    want = np.array([v[key] for v in wide_ed], np.uint8)
    assert {35, 36} <= {v["windows"] for v in wide_ed}
    fold, hs = _run(foldcheck, args, [bytes.fromhex(v["pk"]) for v in wide_ed],
                    [bytes.fromhex(v["sig"]) for v in wide_ed], [bytes.fromhex(v["msg"]) for v in wide_ed], mode)
    _check(fold, hs, want, [v["cat"] for v in wide_ed])


def _s_edges():
    """s values at the comb's edges: 0, 1, L - 1, L, L + 1, 2^252, and the
    radix-2^16 digits 0x7FFF / 0x8000 / 0xFFFF (the signed recoding's carry)
    in the low, a middle and the top position. Honest signatures whose s is
    replaced (so only s = the honest s could verify; s >= L is rejected by
    the s check whatever the comb returns)."""
    vals = [0, 1, L - 1, L, L + 1, 2**252]
    for d in (0x7FFF, 0x8000, 0xFFFF):
        for pos in (0, 7, 15):
            vals.append(d << (16 * pos))
    return vals


@pytest.mark.parametrize("mode", [0, 1])
def test_fold_s_edge_values(foldcheck, mode):
    rng = np.random.default_rng(17)
    vals = _s_edges()
    n = len(vals) + 2
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = [rng.integers(0, 256, 40 + i, dtype=np.uint8).tobytes() for i in range(n)]
    m, off = coracle.pack_msgs(msgs)
    sig = coracle.sign_batch(seeds, m, off, nthreads=2).copy()
    pk = coracle.pubkeys_from_seeds(seeds)
    for i, v in enumerate(vals):
        sig[i, 32:] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    want = coracle.verify_batch(pk, sig, m, off, mode, nthreads=2)
    assert want[-1] == 1 and want[-2] == 1 and want[: len(vals)].sum() == 0
    for args in (["fold"], ["late"]):
        fold, hs = _run(foldcheck, args, pk, sig, msgs, mode)
        _check(fold, hs, want, [hex(v) for v in vals] + ["honest", "honest"])
