"""cmtv_verify_commits_typed on the GPU: many heights of secp256k1, sr25519
and mixed-key validator sets in one call (types.verify_commits), against the
per-height loop of cmtv_verify_commit_typed on the same context and the
reference's loops restated in tests/typed_commit_ref.py (outcome kind, index
and the exact error string).

The batched secp256k1 kernel (k_verify_secp256k1_keyed_batch<KB>: KB
signatures per lane sharing one inversion mod n) is reached on purpose by
contexts opened with CMTV_KEYED_BATCH_MIN_WAVES set; its outcomes must equal
the same call with the knob unset (the one-signature-per-lane kernel) and the
reference. Signatures and reference outcomes are computed once and shared.
"""
import ctypes
import os
import sys
from functools import lru_cache

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_ref as SECP  # noqa: E402
import typed_commit_ref as R  # noqa: E402

from cometbft_amd import _native as N  # noqa: E402
from cometbft_amd import types as T  # noqa: E402

pytestmark = pytest.mark.gpu

CHAIN = "typed-heights"
KINDS = {"full": N.VERIFY_COMMIT, "light": N.VERIFY_COMMIT_LIGHT, "trusting": N.VERIFY_COMMIT_LIGHT_TRUSTING}
KIND_OF = {T.ErrWrongSignature: "wrong_signature", T.ErrNotEnoughVotingPowerSigned: "not_enough_power",
           T.ErrDoubleVote: "double_vote", T.ReferencePanic: "panic", T.ErrInvalidCommitSignatures: "set_size",
           T.ErrInvalidCommitHeight: "height", T.ErrWrongBlockID: "block_id", T.ErrTrustLevel: "trust_level"}


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def open_ctx(cache=0, **env):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cometbft_amd import Context

    with _env(**env):
        ctx = Context(device=0)
    if cache:
        ctx.keyset_cache(cache)
    return ctx


@pytest.fixture(scope="module")
def plain_ctx():
    ctx = open_ctx()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def cache_ctx():
    """cmtv_keyset_cache on, the batching knob unset: registered keys through
    the one-signature-per-lane kernel."""
    ctx = open_ctx(cache=4)
    yield ctx
    ctx.close()


def to_valset(vals):
    return T.ValidatorSet([T.Validator(v.pub_key, v.power, v.priority, v.key_type) for v in vals])


def to_block_id(bid):
    return T.BlockID(bid[0], T.PartSetHeader(bid[1], bid[2]))


def to_commit(commit):
    height, round_, bid, sigs = commit
    return T.Commit(height, round_, to_block_id(bid), [T.CommitSig(s.flag, s.address, s.ts, s.signature) for s in sigs])


def as_outcome(e):
    """None or (kind, message, index) of an exception verify_commits returned."""
    if e is None:
        return None
    idx = e.index if isinstance(e, T.ErrWrongSignature) else -1
    if isinstance(e, T.ErrDoubleVote):
        idx = e.result.sig_index
    return (KIND_OF[type(e)], str(e), idx)


def items_of(heights):
    """heights: [(vals, height, commit)] -> verify_commits items; one ValidatorSet object per distinct set."""
    sets = {}
    out = []
    for vals, height, commit in heights:
        vs = sets.setdefault(id(vals), to_valset(vals))
        out.append((vs, to_block_id(commit[2]), height, to_commit(commit)))
    return out


def many(ctx, kind, heights, chain=CHAIN, trust=(1, 3)):
    got = T.verify_commits(KINDS[kind], chain, items_of(heights), ctx=ctx, trust_level=trust)
    return [as_outcome(e) for e in got]


def loop(ctx, kind, heights, chain=CHAIN, trust=(1, 3)):
    """The per-height loop of cmtv_verify_commit_typed (the parent's only way)."""
    out = []
    for vs, bid, height, cm in items_of(heights):
        try:
            if kind == "full":
                vs.verify_commit(chain, bid, height, cm, ctx=ctx)
            elif kind == "light":
                vs.verify_commit_light(chain, bid, height, cm, ctx=ctx)
            else:
                vs.verify_commit_light_trusting(chain, cm, trust, ctx=ctx)
            out.append(None)
        except (T.CommitError, T.ReferencePanic) as e:
            out.append(as_outcome(e))
    return out


def ref(kind, heights, chain=CHAIN, trust=(1, 3)):
    out = []
    for vals, height, commit in heights:
        vals = list(vals)
        if kind == "full":
            out.append(R.verify_commit(vals, chain, commit[2], height, commit))
        elif kind == "light":
            out.append(R.verify_commit_light(vals, chain, commit[2], height, commit))
        else:
            out.append(R.verify_commit_light_trusting(vals, chain, commit, trust))
    return out


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is not None and w[0] == "block_id":  # the reference restates only the head of that message
            assert g is not None and g[0] == "block_id"
        else:
            assert g == w, (g, w)


@lru_cache(maxsize=None)
def vset(types, start, n):
    return tuple(R.make_vals(list(types) * (n // len(types)), start=start))


@lru_cache(maxsize=None)
def chain_of(types, start, n, h0, count, chain=CHAIN, holes=False):
    vals = vset(types, start, n)
    flags = [R.COMMIT] * n
    if holes:
        flags[3], flags[n - 9] = R.NIL, R.ABSENT
    return tuple((vals, h, R.make_commit(list(vals), chain, h, flags=flags)) for h in range(h0, h0 + count))


def with_sig(entry, idx, sig):
    vals, height, (h, r, bid, sigs) = entry
    sigs = list(sigs)
    s = sigs[idx]
    sigs[idx] = R.Sig(s.flag, s.address, s.ts, sig)
    return (vals, height, (h, r, bid, sigs))


def sig_of(entry, idx):
    return entry[2][3][idx].signature


def flipped(sig, byte=7):
    return sig[:byte] + bytes([sig[byte] ^ 1]) + sig[byte + 1:]


def high_s(sig):
    return sig[:32] + (SECP.N - int.from_bytes(sig[32:], "big")).to_bytes(32, "big")


SECP_T, MIXED_T, ED_T = ("secp256k1",), ("ed25519", "secp256k1", "sr25519", "secp256k1"), ("ed25519",)


@lru_cache(maxsize=None)
def scenario(name):
    a = lambda h0, c, holes=False: list(chain_of(SECP_T, 0, 20, h0, c, holes=holes))  # noqa: E731
    b = lambda h0, c: list(chain_of(SECP_T, 100, 20, h0, c))  # noqa: E731
    mixed = lambda h0, c: list(chain_of(MIXED_T, 200, 20, h0, c, holes=True))  # noqa: E731
    if name == "one_set":  # 6 heights of one 20-validator secp256k1 set
        return a(10, 6)
    if name == "two_sets":  # a change of set after height 3
        return a(10, 3) + b(13, 3)
    if name == "mixed_between":  # a mixed Ed / secp / sr set between two pure ones; nil and absent votes
        return a(20, 2, True) + mixed(22, 2) + a(24, 2, True)
    if name == "wrong_height":  # a commit that fails its preamble in the middle
        hs = a(30, 5)
        hs[2] = (hs[2][0], 99, hs[2][2])
        return hs
    if name == "wrong_sigs":  # a wrong signature at a different index in two heights, of each key type
        hs = mixed(40, 4) + a(44, 2)
        hs[1] = with_sig(hs[1], 5, flipped(sig_of(hs[1], 5)))    # secp256k1
        hs[2] = with_sig(hs[2], 14, flipped(sig_of(hs[2], 14)))  # sr25519
        hs[3] = with_sig(hs[3], 8, flipped(sig_of(hs[3], 8)))    # Ed25519
        hs[5] = with_sig(hs[5], 19, flipped(sig_of(hs[5], 19)))
        return hs
    if name == "single":
        return a(70, 1)
    if name == "decode_rule":
        # an sr25519 validator of a mixed set presents its key with bit 255 set;
        # at the second height its signature is made over those very bytes, so
        # only the decoder's canonical rule makes it wrong
        vals = list(vset(MIXED_T, 200, 20))
        v = vals[6]
        pk = v.pub_key[:31] + bytes([v.pub_key[31] | 0x80])
        vals[6] = R.Val("sr25519", pk, v.power, v.secret)
        hs = [(tuple(vals), h, R.make_commit(vals, CHAIN, h)) for h in (90, 91)]
        msg = R.sign_bytes(CHAIN, 91, 0, hs[1][2][2], hs[1][2][3][6])
        a_log, r = R.SR.expand_mini(v.secret)[0], 98765432109876543210
        sig = R.SR.sign_encoded(a_log, r, msg, pk, R.SR.ristretto_encode(R.SR.scalar_mult(r, R.SR.B)))
        assert v.key_type == "sr25519" and not R.SR.verify(pk, msg, sig)
        assert R.SR.verify_lenient(pk, msg, sig, skip_pk=("canonical",))
        hs[1] = with_sig(hs[1], 6, sig)
        return hs
    raise KeyError(name)


SCENARIOS = ("one_set", "two_sets", "mixed_between", "wrong_height", "wrong_sigs", "single", "decode_rule")


@pytest.mark.parametrize("kind", ("full", "light", "trusting"))
@pytest.mark.parametrize("name", SCENARIOS)
def test_equals_per_height_loop_and_reference(plain_ctx, cache_ctx, name, kind):
    hs = scenario(name)
    want = ref(kind, hs)
    if name == "wrong_sigs" and kind == "full":
        assert [w and w[2] for w in want] == [None, 5, 14, 8, None, 19]
    if name == "decode_rule":  # every loop reaches validator 6
        assert [w and w[2] for w in want] == [6, 6]
    if name == "wrong_height" and kind != "trusting":
        assert [w and w[0] for w in want] == [None, None, "height", None, None]
    for ctx in (plain_ctx, cache_ctx):
        got = many(ctx, kind, hs)
        same(got, want)
        assert got == loop(ctx, kind, hs)


def test_light_trusting_window(cache_ctx):
    """The trusted set against later heights' commits, one short of the trust level."""
    hs = list(chain_of(SECP_T, 0, 20, 60, 3))
    vals = vset(SECP_T, 0, 20)
    sparse = [R.COMMIT if i % 4 == 0 else R.ABSENT for i in range(20)]
    hs.append((vals, 63, R.make_commit(list(vals), CHAIN, 63, flags=sparse)))
    want = ref("trusting", hs, trust=(1, 3))
    assert [w and w[0] for w in want] == [None, None, None, "not_enough_power"]
    got = many(cache_ctx, "trusting", hs, trust=(1, 3))
    same(got, want)
    assert got == loop(cache_ctx, "trusting", hs, trust=(1, 3))


def test_all_ed25519_is_cmtv_verify_commits(plain_ctx):
    """No validator of any commit is non-Ed25519: results, rcs and msg_bufs
    are cmtv_verify_commits' bytes, with key_types NULL, an array of NULLs and
    explicit zeros."""
    hs = list(chain_of(ED_T, 300, 20, 80, 3, holes=True))
    hs[1] = with_sig(hs[1], 2, flipped(sig_of(hs[1], 2)))
    p = T.PackedCommits(N.VERIFY_COMMIT, CHAIN, items_of(hs))
    assert p.kt_arr is None

    def fill():
        for a in (p.res, p.rcs, p.bufs):
            ctypes.memset(a, 0xEE, ctypes.sizeof(a))

    fill()
    p.call(plain_ctx)
    base = (bytes(p.res), bytes(p.rcs), p.bufs.raw)
    assert [p.rcs[i] for i in range(3)] == [N.CMTV_OK, N.CMTV_ECOMMIT, N.CMTV_OK] and p.res[1].sig_index == 2
    zeros = (ctypes.c_uint8 * 20)()
    nulls = (ctypes.POINTER(ctypes.c_uint8) * 3)()
    explicit = (ctypes.POINTER(ctypes.c_uint8) * 3)(*[ctypes.cast(zeros, ctypes.POINTER(ctypes.c_uint8))] * 3)
    for kt in (None, nulls, explicit):
        fill()
        rc = N.lib().cmtv_verify_commits_typed(plain_ctx.handle, p.kind, p.mode, p.cid, len(p.cid), p.n, p.vs_arr, kt,
                                               p.bid_arr, p.heights, p.cm_arr, p.num, p.den, p.res, p.rcs, p.bufs,
                                               p.cap)
        assert rc == N.CMTV_OK
        assert (bytes(p.res), bytes(p.rcs), p.bufs.raw) == base


# (CMTV_KEYED_BATCH_MIN_WAVES, heights, validators, KB): with every vote for
# the block the batch is heights x validators signatures, signature h * V + i
# in round (h * V + i) // lanes of lane (h * V + i) % lanes, lanes = 64 x workgroups:
#   1, 3 x 70  = 210: KB 8, one workgroup, rounds 0-3 (the last partial), 4-7 wholly inactive
#   1, 13 x 40 = 520: KB 8, two workgroups, round 4 has 8 signatures
#   2, 5 x 60  = 300: KB 4, two workgroups, round 2 partial
BATCHED = ((1, 3, 70, 8), (1, 13, 40, 8), (2, 5, 60, 4))


def kb_for(n, min_waves):
    kb = 1
    while kb < 8 and n > (min_waves - 1) * 64 * (kb * 2):
        kb *= 2
    return kb if kb >= 4 else 1


INF_IDX = 12  # batched_heights' validator whose signature at the fourth height sums to infinity


@lru_cache(maxsize=None)
def batched_heights(n_heights, n_vals):
    """All votes for the block; the last validator holds a key the parser
    rejects (every height's last signature is wrong); a flipped signature, an
    s = 0, an s = n and a high-S twin at different indices of different
    heights, the twin in a height with a later flipped signature. With more
    than three heights, validator 12's private key is -e / r for its own
    message e of the fourth height and r = 5: it signs honestly everywhere
    else, and its (r, s) there makes [u1]G + [u2]Q the point at infinity."""
    good = list(R.make_vals(["secp256k1"] * n_vals, start=400))
    last = good[-1]
    good[-1] = R.Val("secp256k1", bytes([5]) + last.pub_key[1:], last.power, last.secret)
    assert SECP.parse_pubkey(good[-1].pub_key) is None
    if n_heights > 3:
        msg = R.sign_bytes(CHAIN, 503, 0, R.block_id_for(503), R.Sig(R.COMMIT, b"", R.timestamp_for(INF_IDX)))
        d = (-SECP.msg_scalar(msg) * pow(5, SECP.N - 2, SECP.N) % SECP.N).to_bytes(32, "big")
        good[INF_IDX] = R.Val("secp256k1", SECP.pubkey_from_priv(d), good[INF_IDX].power, d)
    vals = tuple(good)
    hs = [(vals, h, R.make_commit(list(vals), CHAIN, h)) for h in range(500, 500 + n_heights)]
    zero_s = lambda sig: sig[:32] + bytes(32)  # noqa: E731
    n_s = lambda sig: sig[:32] + SECP.N.to_bytes(32, "big")  # noqa: E731
    hs[0] = with_sig(hs[0], 7, high_s(sig_of(hs[0], 7)))
    hs[0] = with_sig(hs[0], n_vals - 2, flipped(sig_of(hs[0], n_vals - 2)))
    hs[1] = with_sig(hs[1], 33, zero_s(sig_of(hs[1], 33)))
    hs[2] = with_sig(hs[2], 21, n_s(sig_of(hs[2], 21)))
    if n_heights > 3:
        hs[n_heights - 1] = with_sig(hs[n_heights - 1], 2, flipped(sig_of(hs[n_heights - 1], 2), 40))
        inf = (5).to_bytes(32, "big") + (SECP.HALF_N - 1).to_bytes(32, "big")
        assert SECP.verify(good[INF_IDX].pub_key, msg, sig_of(hs[3], INF_IDX))
        assert not SECP.verify(good[INF_IDX].pub_key, msg, inf)
        assert SECP.verify_without_z_test(good[INF_IDX].pub_key, msg, inf)
        hs[3] = with_sig(hs[3], INF_IDX, inf)
    return tuple(hs)


@pytest.mark.parametrize("min_waves,n_heights,n_vals,kb", BATCHED)
def test_batched_kernel(cache_ctx, min_waves, n_heights, n_vals, kb):
    n = n_heights * n_vals
    assert kb_for(n, min_waves) == kb
    lanes = 64 * ((n + 64 * kb - 1) // (64 * kb))
    hs = list(batched_heights(n_heights, n_vals))
    # at least one lane holds an invalid and a valid signature in different rounds
    bad = {0 * n_vals + 7, 0 * n_vals + n_vals - 2, 1 * n_vals + 33, 2 * n_vals + 21} | \
        {h * n_vals + n_vals - 1 for h in range(n_heights)} | ({3 * n_vals + INF_IDX} if n_heights > 3 else set())
    assert any(q not in bad and q % lanes == p % lanes for p in bad for q in range(n))
    want = ref("full", hs)
    assert [w[2] for w in want[:3]] == [7, 33, 21] and all(w[2] == n_vals - 1 for w in want[4:-1])
    assert n_heights == 3 or want[3][2] == INF_IDX  # the infinity signature is the fourth height's first wrong one
    ctx = open_ctx(cache=4, CMTV_KEYED_BATCH_MIN_WAVES=min_waves)
    try:
        for kind in ("full", "light"):
            s0 = ctx.stats()
            got = many(ctx, kind, hs)
            s1 = ctx.stats()
            if kind == "full":  # (VerifyCommitLight plans fewer signatures: whichever kernel their count gives)
                assert s1["secp_batch_launches"] - s0["secp_batch_launches"] == 1
            assert s1["keyed_launches"] - s0["keyed_launches"] == 1
            same(got, want if kind == "full" else ref("light", hs))
            # the knob unset: the one-signature-per-lane kernel
            c0 = cache_ctx.stats()
            assert got == many(cache_ctx, kind, hs)
            c1 = cache_ctx.stats()
            assert c1["secp_batch_launches"] == c0["secp_batch_launches"] and c1["keyed_launches"] > c0["keyed_launches"]
        # cmtv_verify_commit_typed never batches, whatever the knob says: the
        # first height alone is one one-signature-per-lane launch
        s0 = ctx.stats()
        same(loop(ctx, "full", hs[:1]), want[:1])
        s1 = ctx.stats()
        assert s1["secp_batch_launches"] == s0["secp_batch_launches"]
        assert s1["keyed_launches"] - s0["keyed_launches"] == 1
    finally:
        ctx.close()


def test_two_registered_sets_in_order():
    """More groups than the cache holds (cmtv_keyset_cache(ctx, 1)): A, B, A
    run one after another, each by its own registered keys."""
    hs = list(chain_of(SECP_T, 0, 20, 10, 3)) + list(chain_of(SECP_T, 100, 20, 13, 3)) + list(chain_of(SECP_T, 0, 20, 16, 2))
    hs[4] = with_sig(hs[4], 11, flipped(sig_of(hs[4], 11)))
    hs[7] = with_sig(hs[7], 0, flipped(sig_of(hs[7], 0)))
    want = ref("full", hs)
    assert [w and w[2] for w in want] == [None, None, None, None, 11, None, None, 0]
    ctx = open_ctx(cache=1, CMTV_KEYED_BATCH_MIN_WAVES=1)
    try:
        s0 = ctx.stats()
        same(many(ctx, "full", hs), want)
        s1 = ctx.stats()
        assert s1["keyed_launches"] - s0["keyed_launches"] == 3
        assert s1["secp_batch_launches"] - s0["secp_batch_launches"] == 3
    finally:
        ctx.close()


def test_long_chain_id_takes_the_non_fused_route():
    """Messages above 192 bytes: k_sign_bytes and the message-reading kernel,
    no batched launch even with the knob at 1, the same outcomes."""
    chain = "y" * 150
    hs = list(chain_of(SECP_T, 0, 20, 10, 4, chain=chain))
    hs[2] = with_sig(hs[2], 6, flipped(sig_of(hs[2], 6)))
    want = ref("full", hs, chain=chain)
    assert [w and w[2] for w in want] == [None, None, 6, None]
    ctx = open_ctx(cache=4, CMTV_KEYED_BATCH_MIN_WAVES=1)
    try:
        s0 = ctx.stats()
        same(many(ctx, "full", hs, chain=chain), want)
        s1 = ctx.stats()
        assert s1["secp_batch_launches"] == s0["secp_batch_launches"]
        assert s1["keyed_launches"] > s0["keyed_launches"]
    finally:
        ctx.close()


def test_library_error_is_the_calls_return():
    """CMTV_FAULT_AT: the failed launch's CMTV_EHIP comes back as the call's
    return value, and the context keeps working."""
    hs = list(scenario("one_set"))
    ctx = open_ctx(CMTV_FAULT_AT=1)
    try:
        with pytest.raises(N.CmtvError) as ei:
            many(ctx, "full", hs)
        assert ei.value.code == N.CMTV_EHIP
        same(many(ctx, "full", hs), [None] * 6)
    finally:
        ctx.close()
