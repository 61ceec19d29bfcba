"""cmtv_verify_commit_typed on the GPU: commits of secp256k1, sr25519 and
mixed-key validator sets through ValidatorSet.verify_commit*, against the
reference's loops restated in tests/typed_commit_ref.py (outcome kind, index
and the exact error string).

Both secp256k1 routes run: the templated kernels (every message at most
kSbFuseMaxMsg = 192 bytes) and k_sign_bytes + the message-reading kernels (a
150-byte chain id), by key bytes and, with cmtv_keyset_cache on, by
registered keys. References are computed once per (set, commit) and shared.
"""
import ctypes
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_ref as SECP  # noqa: E402
import typed_commit_ref as R  # noqa: E402

from cometbft_amd import _native as N  # noqa: E402
from cometbft_amd import types as T  # noqa: E402

pytestmark = pytest.mark.gpu

HEIGHT = 77
CHAINS = {"empty": "", "c": "c", "x50": "x" * 50, "y150": "y" * 150}
# n -> the chain id its sweep uses: every size meets a different message
# length, and 65 (one lane into a second workgroup) the non-fused route too
CHAIN_OF_N = {1: "empty", 63: "c", 64: "x50", 65: "y150", 130: "x50"}


@pytest.fixture(scope="module")
def cache_ctx():
    """A context of its own with cmtv_keyset_cache on (the session context's
    cache stays as the other tests expect it)."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cometbft_amd import Context

    ctx = Context(device=0)
    ctx.keyset_cache(4)
    yield ctx
    ctx.close()


def to_valset(vals):
    return T.ValidatorSet([T.Validator(v.pub_key, v.power, v.priority, v.key_type) for v in vals])


def to_commit(commit):
    height, round_, bid, sigs = commit
    css = [T.CommitSig(s.flag, s.address, s.ts, s.signature) for s in sigs]
    return T.Commit(height, round_, to_block_id(bid), css)


def to_block_id(bid):
    return T.BlockID(bid[0], T.PartSetHeader(bid[1], bid[2]))


KIND_OF = {T.ErrWrongSignature: "wrong_signature", T.ErrNotEnoughVotingPowerSigned: "not_enough_power",
           T.ErrDoubleVote: "double_vote", T.ReferencePanic: "panic", T.ErrInvalidCommitSignatures: "set_size",
           T.ErrInvalidCommitHeight: "height", T.ErrWrongBlockID: "block_id", T.ErrTrustLevel: "trust_level"}


def outcome(fn):
    """None or (kind, message, index) of a ValidatorSet.verify_* call."""
    try:
        fn()
    except (T.CommitError, T.ReferencePanic) as e:
        idx = e.index if isinstance(e, T.ErrWrongSignature) else -1
        if isinstance(e, T.ErrDoubleVote):
            idx = e.result.sig_index
        return (KIND_OF[type(e)], str(e), idx)
    return None


def run(kind, ctx, vals, chain, commit, trust=(1, 3)):
    vs, cm, bid = to_valset(vals), to_commit(commit), to_block_id(commit[2])
    if kind == "full":
        return outcome(lambda: vs.verify_commit(chain, bid, HEIGHT, cm, ctx=ctx))
    if kind == "light":
        return outcome(lambda: vs.verify_commit_light(chain, bid, HEIGHT, cm, ctx=ctx))
    return outcome(lambda: vs.verify_commit_light_trusting(chain, cm, trust, ctx=ctx))


def ref(kind, vals, chain, commit, trust=(1, 3)):
    want = {"full": lambda: R.verify_commit(vals, chain, commit[2], HEIGHT, commit),
            "light": lambda: R.verify_commit_light(vals, chain, commit[2], HEIGHT, commit),
            "trusting": lambda: R.verify_commit_light_trusting(vals, chain, commit, trust)}[kind]()
    return want


def check(kind, ctx, vals, chain, commit, trust=(1, 3)):
    got, want = run(kind, ctx, vals, chain, commit, trust), ref(kind, vals, chain, commit, trust)
    if want is not None and want[0] == "panic":  # the panic's index is the library's own
        assert got is not None and got[:2] == want[:2], (got, want)
    else:
        assert got == want, (got, want)
    return got


@lru_cache(maxsize=None)
def secp_set(n):
    return tuple(R.make_vals(["secp256k1"] * n))


@lru_cache(maxsize=None)
def secp_commit(n, chain_name, with_flags=True):
    """A good commit of secp_set(n): with_flags puts a nil vote and an absent
    one in (where n allows) -- every other validator signs for the block."""
    flags = [R.COMMIT] * n
    if with_flags and n >= 63:
        flags[5], flags[11] = R.NIL, R.ABSENT
    return R.make_commit(list(secp_set(n)), CHAINS[chain_name], HEIGHT, flags=flags)


def with_sig(commit, idx, sig=None, **kw):
    """commit with signature idx replaced (a copy)."""
    h, r, bid, sigs = commit
    sigs = list(sigs)
    s = sigs[idx]
    sigs[idx] = R.Sig(kw.get("flag", s.flag), kw.get("address", s.address), kw.get("ts", s.ts),
                      s.signature if sig is None else sig)
    return (h, r, bid, sigs)


def flipped(sig, byte=7):
    return sig[:byte] + bytes([sig[byte] ^ 1]) + sig[byte + 1:]


def high_s(sig):
    s = int.from_bytes(sig[32:], "big")
    return sig[:32] + (SECP.N - s).to_bytes(32, "big")


# ------------------------------------------------------------------ all secp256k1

@pytest.mark.parametrize("cached", [False, True], ids=["nocache", "cache"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_secp_verify_commit_sizes(gpu_ctx, cache_ctx, n, cached):
    ctx = cache_ctx if cached else gpu_ctx
    vals, chain = list(secp_set(n)), CHAIN_OF_N[n]
    good = secp_commit(n, chain)
    s0 = ctx.stats()
    assert check("full", ctx, vals, CHAINS[chain], good) is None
    s1 = ctx.stats()
    # the route: lanes build the messages unless the chain id makes them too long
    assert (s1["fused_sign_bytes"] > s0["fused_sign_bytes"]) == (chain != "y150")
    assert (s1["keyed_launches"] > s0["keyed_launches"]) == cached
    if cached:  # the registered set is found again: the same outcome
        assert check("full", ctx, vals, CHAINS[chain], good) is None
    # the last signature wrong: the error is its own, whatever workgroup and
    # lane it falls in
    bad = with_sig(good, n - 1, flipped(good[3][n - 1].signature))
    got = check("full", ctx, vals, CHAINS[chain], bad)
    assert got[0] == "wrong_signature" and got[2] == n - 1
    if cached:
        assert check("full", ctx, vals, CHAINS[chain], bad) == got
    # every validator signing for the block: the plan is the commit itself
    # and the layer hands the caller's arrays to the batch
    full = secp_commit(n, chain, False)
    assert check("full", ctx, vals, CHAINS[chain], full) is None
    bad = with_sig(full, n // 2, flipped(full[3][n // 2].signature))
    assert check("full", ctx, vals, CHAINS[chain], bad)[2] == n // 2


@pytest.mark.parametrize("cached", [False, True], ids=["nocache", "cache"])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_secp_chain_ids(gpu_ctx, cache_ctx, chain, cached):
    ctx = cache_ctx if cached else gpu_ctx
    n = 65
    vals, good = list(secp_set(n)), secp_commit(n, chain)
    assert check("full", ctx, vals, CHAINS[chain], good) is None
    # a signature over another chain id's sign-bytes
    other = secp_commit(n, "c" if chain != "c" else "empty")
    bad = with_sig(good, 40, other[3][40].signature)
    assert check("full", ctx, vals, CHAINS[chain], bad)[2] == 40


@pytest.mark.parametrize("cached", [False, True], ids=["nocache", "cache"])
def test_secp_light_never_reaches_a_late_bad_signature(gpu_ctx, cache_ctx, cached):
    ctx = cache_ctx if cached else gpu_ctx
    n = 130
    vals, good = list(secp_set(n)), secp_commit(n, "x50")
    late = with_sig(good, n - 2, flipped(good[3][n - 2].signature))
    assert check("light", ctx, vals, CHAINS["x50"], late) is None
    assert check("full", ctx, vals, CHAINS["x50"], late)[2] == n - 2
    early = with_sig(good, 3, flipped(good[3][3].signature))
    assert check("light", ctx, vals, CHAINS["x50"], early)[2] == 3


@pytest.mark.parametrize("cached", [False, True], ids=["nocache", "cache"])
def test_secp_light_trusting(gpu_ctx, cache_ctx, cached):
    """Addresses are RIPEMD160(SHA256(key)); the loop returns at 1/3; a double
    vote prints the key as PubKeySecp256k1{...}."""
    ctx = cache_ctx if cached else gpu_ctx
    n = 64
    vals, good = list(secp_set(n)), secp_commit(n, "c", with_flags=False)
    chain = CHAINS["c"]
    assert check("trusting", ctx, vals, chain, good) is None
    # past the 1/3 mark nothing is examined
    late = with_sig(good, 40, flipped(good[3][40].signature))
    assert check("trusting", ctx, vals, chain, late) is None
    early = with_sig(good, 2, flipped(good[3][2].signature))
    assert check("trusting", ctx, vals, chain, early)[2] == 2
    # signature 4 carries validator 1's address again
    dv = with_sig(good, 4, address=vals[1].address)
    got = check("trusting", ctx, vals, chain, dv)
    assert got[0] == "double_vote" and "PubKeySecp256k1{" + vals[1].pub_key.hex().upper() + "}" in got[1]
    # an address of the SHA256[:20] kind matches nobody: every vote is skipped
    import hashlib
    stray = good
    for i in range(n):
        stray = with_sig(stray, i, address=hashlib.sha256(vals[i].pub_key).digest()[:20])
    assert check("trusting", ctx, vals, chain, stray)[0] == "not_enough_power"


SECP_BAD = ["zero_sec", "zero_nanos", "high_s", "sig63", "prefix4", "off_curve", "key32", "infinity"]


@pytest.mark.parametrize("cached", [False, True], ids=["nocache", "cache"])
@pytest.mark.parametrize("case", SECP_BAD)
def test_secp_signature_and_key_cases(gpu_ctx, cache_ctx, case, cached):
    """Each bad input is "wrong signature (#i)" with the exact hex, never a
    panic; zero seconds / nanos (fields the encoder omits) verify."""
    ctx = cache_ctx if cached else gpu_ctx
    n, i = 65, 64
    vals, chain = list(secp_set(n)), CHAINS["x50"]
    good = secp_commit(n, "x50")
    if case in ("zero_sec", "zero_nanos"):
        ts = (0, 123) if case == "zero_sec" else (1700000000, 0)
        s = R.Sig(R.COMMIT, vals[i].address, ts)
        s.signature = R.sign("secp256k1", vals[i].secret, R.sign_bytes(chain, HEIGHT, 0, good[2], s))
        assert check("full", ctx, vals, chain, with_sig(good, i, s.signature, ts=ts)) is None
        # ... and not under the timestamp it was not signed with
        assert check("full", ctx, vals, chain, with_sig(good, i, s.signature))[2] == i
        return
    commit = good
    if case == "high_s":
        commit = with_sig(good, i, high_s(good[3][i].signature))
    elif case == "sig63":
        commit = with_sig(good, i, good[3][i].signature[:63])
    elif case == "infinity":
        # the key [-e / r]G: [u1]G + [u2]Q is the point at infinity, which
        # X = r Z alone accepts (0 = r * 0); r + n < p
        msg, r = R.sign_bytes(chain, HEIGHT, 0, good[2], good[3][i]), 5
        d = -SECP.msg_scalar(msg) * pow(r, SECP.N - 2, SECP.N) % SECP.N
        pk, sig = SECP.pubkey_from_priv(d.to_bytes(32, "big")), r.to_bytes(32, "big") + SECP.HALF_N.to_bytes(32, "big")
        assert SECP.verify_without_z_test(pk, msg, sig) and not SECP.verify(pk, msg, sig)
        vals = vals[:i] + [R.Val("secp256k1", pk, vals[i].power, vals[i].secret)] + vals[i + 1:]
        commit = with_sig(good, i, sig)
    else:
        pk = vals[i].pub_key
        if case == "prefix4":
            pk = b"\x04" + pk[1:]
        elif case == "off_curve":
            x = int.from_bytes(pk[1:], "big")
            while SECP.lift_x(x, 0) is not None:
                x += 1
            pk = pk[:1] + x.to_bytes(32, "big")
        else:
            pk = pk[1:]
        vals = vals[:i] + [R.Val("secp256k1", pk, vals[i].power, vals[i].secret)] + vals[i + 1:]
    got = check("full", ctx, vals, chain, commit)
    assert got == ("wrong_signature",
                   "wrong signature (#%d): %s" % (i, commit[3][i].signature.hex().upper()), i)


# ------------------------------------------------------------------ all sr25519

@pytest.fixture(scope="module")
def sr_case():
    vals = R.make_vals(["sr25519"] * 65)
    return vals, R.make_commit(vals, "sr-chain", HEIGHT)


@pytest.mark.parametrize("case", ["good", "flipped", "key31", "bit255", "negative_r"])
def test_sr25519_set(gpu_ctx, sr_case, case):
    vals, commit = sr_case
    if case == "flipped":
        commit = with_sig(commit, 33, flipped(commit[3][33].signature))
    if case in ("bit255", "negative_r"):
        # validator 9 presents another encoding of its key (bit 255 set), or of
        # R (p - s), and signs over those bytes: only the decoder's canonical /
        # non-negative rule makes the signature wrong
        msg = R.sign_bytes("sr-chain", HEIGHT, 0, commit[2], commit[3][9])
        a, r = R.SR.expand_mini(vals[9].secret)[0], 12345678901234567890
        pk, rb = vals[9].pub_key, R.SR.ristretto_encode(R.SR.scalar_mult(r, R.SR.B))
        if case == "bit255":
            pk, skip = pk[:31] + bytes([pk[31] | 0x80]), {"skip_pk": ("canonical",)}
            vals = vals[:9] + [R.Val("sr25519", pk, vals[9].power)] + vals[10:]
        else:
            rb, skip = (R.SR.P - int.from_bytes(rb, "little")).to_bytes(32, "little"), {"skip_r": ("nonneg_s",)}
        sig = R.SR.sign_encoded(a, r, msg, pk, rb)
        assert R.SR.verify_lenient(pk, msg, sig, **skip) and not R.SR.verify(pk, msg, sig)
        commit = with_sig(commit, 9, sig)
    if case == "key31":  # zero-padded to 32 bytes: another key, so the signature is wrong
        vals = vals[:9] + [R.Val("sr25519", vals[9].pub_key[:31], vals[9].power)] + vals[10:]
    got = check("full", gpu_ctx, vals, "sr-chain", commit)
    assert (got is None) == (case == "good")
    if case != "good":
        assert got[0] == "wrong_signature" and got[2] == (33 if case == "flipped" else 9)


def test_sr25519_short_key_that_pads_to_itself(gpu_ctx):
    """A key whose last byte is zero, given without it: the reference pads it
    back, and the signature verifies."""
    i = 0
    while R.keypair("sr25519", 1000 + i)[1][31] != 0:
        i += 1
        if i > 4096:
            pytest.fail("no sr25519 key ending in a zero byte among 4096")
    secret, pk = R.keypair("sr25519", 1000 + i)
    vals = R.make_vals(["sr25519"] * 3)
    vals[1] = R.Val("sr25519", pk, 10, secret)
    commit = R.make_commit(vals, "sr-chain", HEIGHT)
    vals[1] = R.Val("sr25519", pk[:31], 10, secret)
    assert check("full", gpu_ctx, vals, "sr-chain", commit) is None


# ------------------------------------------------------------------ mixed

MIXED_TYPES = ["ed25519", "secp256k1", "sr25519"] * 22


@pytest.fixture(scope="module")
def mixed_case():
    vals = R.make_vals(MIXED_TYPES)
    flags = [R.COMMIT] * 66
    flags[7], flags[8], flags[20] = R.NIL, R.ABSENT, R.NIL
    return vals, R.make_commit(vals, "mixed-chain", HEIGHT, flags=flags)


@pytest.mark.parametrize("cached", [False, True], ids=["nocache", "cache"])
@pytest.mark.parametrize("kind", ["full", "light", "trusting"])
def test_mixed_good(gpu_ctx, cache_ctx, mixed_case, kind, cached):
    vals, commit = mixed_case
    assert check(kind, cache_ctx if cached else gpu_ctx, vals, "mixed-chain", commit) is None


@pytest.mark.parametrize("bad", [(30,), (31,), (32,), (62, 31, 30), (32, 60), (61, 33)])
def test_mixed_first_error_is_in_commit_order(gpu_ctx, mixed_case, bad):
    """A bad signature in each type's part (30 Ed25519, 31 secp256k1, 32
    sr25519), and several at once: the error is the lowest commit index."""
    vals, commit = mixed_case
    for i in bad:
        commit = with_sig(commit, i, flipped(commit[3][i].signature))
    got = check("full", gpu_ctx, vals, "mixed-chain", commit)
    assert got[0] == "wrong_signature" and got[2] == min(bad)
    got = check("light", gpu_ctx, vals, "mixed-chain", commit)
    assert got[0] == "wrong_signature" and got[2] == min(bad)


def test_mixed_short_ed25519_key_still_panics(gpu_ctx, mixed_case):
    vals, commit = mixed_case
    vals = vals[:12] + [R.Val("ed25519", vals[12].pub_key[:31], 10)] + vals[13:]
    got = check("full", gpu_ctx, vals, "mixed-chain", commit)
    assert got[0] == "panic" and got[1] == "ed25519: bad public key length: 31"
    # ... after the signature-length check: a 63-byte signature there is a wrong signature
    short = with_sig(commit, 12, commit[3][12].signature[:63])
    assert check("full", gpu_ctx, vals, "mixed-chain", short)[0] == "wrong_signature"
    # ... and a wrong signature before it wins
    assert check("full", gpu_ctx, vals, "mixed-chain", with_sig(commit, 4, flipped(commit[3][4].signature)))[2] == 4


# ------------------------------------------------------------------ the C entry point itself

def _c_args(vals, commit):
    vs, keep_v = to_valset(vals)._pack()
    cm, keep_c = T._pack_commit(to_commit(commit))
    bid, keep_b = to_block_id(commit[2])._c()
    return vs, cm, bid, (keep_v, keep_c, keep_b)


def _call(ctx, vs, cm, bid, chain, types=None, kind=N.VERIFY_COMMIT, typed=True):
    res = N.cmtv_commit_result()
    buf = ctypes.create_string_buffer(1024)
    cid = chain.encode()
    if typed:
        kt = None if types is None else np.ascontiguousarray(types, np.uint8).ctypes.data_as(
            ctypes.POINTER(ctypes.c_uint8))
        rc = N.lib().cmtv_verify_commit_typed(ctx.handle, kind, 0, cid, len(cid), ctypes.byref(vs), kt,
                                              ctypes.byref(bid), HEIGHT, ctypes.byref(cm), 1, 3, ctypes.byref(res),
                                              buf, len(buf))
    else:
        rc = N.lib().cmtv_verify_commit(ctx.handle, kind, 0, cid, len(cid), ctypes.byref(vs), ctypes.byref(bid),
                                        HEIGHT, ctypes.byref(cm), 1, 3, ctypes.byref(res), buf, len(buf))
    return rc, bytes(res), buf.value


@pytest.mark.parametrize("bad_at", [None, 5])  # 5: before LightTrusting's 1/3 is reached
def test_all_ed25519_is_the_existing_entry_point(gpu_ctx, bad_at):
    """key_types NULL and all-zero types: byte-identical cmtv_commit_result
    and message to cmtv_verify_commit, on a good commit and on an error."""
    vals = R.make_vals(["ed25519"] * 40)
    commit = R.make_commit(vals, "ed-chain", HEIGHT)
    if bad_at is not None:
        commit = with_sig(commit, bad_at, flipped(commit[3][bad_at].signature))
    vs, cm, bid, keep = _c_args(vals, commit)
    for kind in (N.VERIFY_COMMIT, N.VERIFY_COMMIT_LIGHT, N.VERIFY_COMMIT_LIGHT_TRUSTING):
        want = _call(gpu_ctx, vs, cm, bid, "ed-chain", kind=kind, typed=False)
        assert want[0] == (N.CMTV_OK if bad_at is None else N.CMTV_ECOMMIT)
        assert _call(gpu_ctx, vs, cm, bid, "ed-chain", None, kind) == want
        assert _call(gpu_ctx, vs, cm, bid, "ed-chain", np.zeros(40, np.uint8), kind) == want


def test_argument_checks(gpu_ctx):
    """A type above 2 and a 65-byte secp256k1 key are CMTV_EINVAL (on a
    context and a commit that verify otherwise)."""
    vals, commit = list(secp_set(63)), secp_commit(63, "c")
    vs, cm, bid, keep = _c_args(vals, commit)
    ones = np.ones(63, np.uint8)
    assert _call(gpu_ctx, vs, cm, bid, "c", ones)[0] == N.CMTV_OK
    three = ones.copy()
    three[62] = 3
    assert _call(gpu_ctx, vs, cm, bid, "c", three)[0] == N.CMTV_EINVAL
    q = SECP.to_affine(SECP.parse_pubkey(vals[10].pub_key))
    unc = b"\x04" + q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")
    vals65 = vals[:10] + [R.Val("secp256k1", unc, 10)] + vals[11:]
    vs, cm, bid, keep = _c_args(vals65, commit)
    assert _call(gpu_ctx, vs, cm, bid, "c", ones)[0] == N.CMTV_EINVAL
    # the same key typed Ed25519 is no argument error (it is the reference's panic)
    ed = ones.copy()
    ed[10] = 0
    assert _call(gpu_ctx, vs, cm, bid, "c", ed)[0] == N.CMTV_ECOMMIT


def test_keyset_cache_off_frees_and_reregisters(cache_ctx):
    """cmtv_keyset_cache(ctx, 0) drops the registered secp256k1 sets; turned
    on again the next call registers anew."""
    vals, good = list(secp_set(63)), secp_commit(63, "c")
    assert check("full", cache_ctx, vals, "c", good) is None
    cache_ctx.keyset_cache(0)
    s0 = cache_ctx.stats()
    assert check("full", cache_ctx, vals, "c", good) is None
    assert cache_ctx.stats()["keyed_launches"] == s0["keyed_launches"]
    cache_ctx.keyset_cache(4)
    assert check("full", cache_ctx, vals, "c", good) is None
    assert cache_ctx.stats()["keyed_launches"] > s0["keyed_launches"]
