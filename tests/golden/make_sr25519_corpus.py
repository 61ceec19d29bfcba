"""Generate the sr25519 edge-case corpus (tests/golden/sr25519_corpus.json).

Every vector holds (pk, sig, msg) and the verdict of
sr25519.PubKey.VerifySignature (/root/reference/crypto/sr25519/pubkey.go:34-60)
computed by the big-int restatement `oracle/sr25519_ref.py`, cross-checked at
generation time against the C restatement (oracle/liboracle.so). Also holds
the published vectors that pin the restatement (ristretto255 RFC 9496 A.1
multiples of B, the merlin simple-transcript challenge, one schnorrkel
verification vector) so the CPU tests need neither the generator nor the
network.

Categories:
  honest          valid signatures, message lengths 0..300 (incl. the 42 / 116 /
                  161-byte CanonicalVote sizes)
  bitflip         one flipped bit in R, s or the message
  no_marker       valid signature with the schnorrkel marker bit (sig[63] & 0x80) cleared
  s_range         s >= L with the marker set (s + L, L, 2^255 - 1, ...)
  pk_encoding     non-canonical / negative / non-square / bit-255 public keys
  r_encoding      the same encodings in R
  identity_pk     the all-zero key (the identity) with s = r: valid
  rfc_bad         RFC 9496 A.2-style invalid encodings as pk and as R
  random          random bytes
  decode_pk, decode_r
                  one ristretto255 decode rule each ("rule"), as the key and as
                  R: the strict verdict is invalid and the verdict of a verifier
                  WITHOUT that one rule (oracle/sr25519_ref.py verify_lenient)
                  is valid; both are asserted here and again from the JSON in
                  tests/test_sr25519_oracle.py. The pk_encoding / r_encoding /
                  rfc_bad vectors pair a bad encoding with a signature made for
                  other bytes, so the challenge changes and any decoder rejects
                  them; these are signed over the alternative encoding e itself
                  by a signer who knows the log a of the point e decodes to
                  without the rule (key: transcript over e, s = r + k a; R: e in
                  the transcript and the signature):
                    canonical   p (the identity's ed ff .. 7f; of s + p, s < 19,
                                the only one in a coset with a known log), and
                                bit 255 set on an honest encoding
                    nonneg_s    p - s (odd)
                    nonneg_t    the coset's other even representatives among
                                1/s, -1/s and those times sqrt(-1) that decode
                                with t negative
                    nonzero_y   s = p - 1 (ec ff .. 7f): a point of order 4, in
                                the identity's coset
                  was_square has no such vector: without the rule a non-square
                  encoding gives coordinates off the curve, on which the
                  addition formulas are no group law, and was_square_search
                  finds none of its candidates (even s < 1000, RFC_BAD) accepted
                  under the two signatures that need no discrete log. The rule
                  is pinned at the primitive (tests/dev/devcases.py
                  check_ristretto_decode).

    python tests/golden/make_sr25519_corpus.py [--out tests/golden/sr25519_corpus.json]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from oracle import coracle as C  # noqa: E402
from oracle import sr25519_ref as S  # noqa: E402
from oracle import signbytes as SB  # noqa: E402

SEED = 25519
P, L = S.P, S.L
PINNED_RULES = ("canonical", "nonneg_s", "nonneg_t", "nonzero_y")  # by decode_pk / decode_r vectors

RISTRETTO_MULTIPLES = [  # RFC 9496 appendix A.1: encodings of [i]B, i = 0..8
    "0000000000000000000000000000000000000000000000000000000000000000",
    "e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76",
    "6a493210f7499cd17fecb510ae0cea23a110e8d5b901f8acadd3095c73a3b919",
    "94741f5d5d52755ece4f23f044ee27d5d1ea1e2bd196b462166b16152a9d0259",
    "da80862773358b466ffadfe0b3293ab3d9fd53c5ea6c955358f568322daf6a57",
    "e882b131016b52c1d3337080187cf768423efccbb517bb495ab812c4160ff44e",
    "f64746d3c92b13050ed8d80236a7f0007c3b3f962f5ba793d19a601ebb1df403",
    "44f53520926ec81fbd5a387845beb7df85a96a24ece18738bdcfa6a7822a176d",
    "903293d8f2287ebe10e2374dc1a53e0bc887e592699f02d077d5263cdd55601c",
]
MERLIN_SIMPLE = {  # gtank/merlin merlin_test.go TestSimpleTranscript
    "label": "test protocol", "msg_label": "some label", "msg": "some data",
    "challenge_label": "challenge",
    "challenge": "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615",
}
SCHNORRKEL_VECTOR = {  # a schnorrkel-rs signature carried in go-schnorrkel's tests
    "context": "substrate", "msg": "this is a message",
    "pk": "46ebddef8cd9bb167dc30878d7113b7e168e6f0646beffd77d69d39bad76b47a",
    "sig": "4e172314444b8f820bb54c22e95076f220ed25373e5c178234aa6c211d29271244b947e3ff3418ff6b45fd1df1140c8cbff69fc58ee6dc96df70936a2bb74b82",
}
RFC_BAD = [  # invalid ristretto255 encodings (non-canonical, negative, non-square, ...)
    "00ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
    "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
    "f3ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
    "edffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
    "0100000000000000000000000000000000000000000000000000000000000000",
    "01ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
    "ed57ffd8c914fb201471d1c3d245ce3c746fcbe63a3679d51b6a516ebebe0e20",
    "c34c4e1826e5d403b78e246e88aa051c36ccf0aafebffe137d148a2bf9104562",
    "c940e5a4404157cfb1628b108db051a8d439e1a421394ec4ebccb9ec92a8ac78",
    "47cfc5497c53dc8e61c91d17fd626ffb1c49e2bca94eed052281b510b1117a24",
    "f1c6165d33367351b0da8f6e4511010c68174a03b6581212c71c0e1d026c3c72",
    "87260f7a2f12495118360f02c26a470f450dadf34a413d21042b43b9d93e1309",
    "26948d35ca62e643e26a83177332e6b6afeb9d08e4268b650f1f5bbd8d81d371",
    "4eac077a713c57b4f4397629a4145982c661f48044dd3f96427d40b147d9742f",
    "de6a7b00deadc788eb6b6c8d20c0ae96c2f2019078fa604fee5b87d6e989ad7b",
    "bcab477be20861e01e4a0e295284146a510150d9817763caf1a6f4b422d67042",
    "2a292df7e32cababbd9de088d1d1abec9fc0440f637ed2fba145094dc14bea08",
    "f4a9e534fc0d216c44b218fa0c42d99635a0127ee2e53c712f70609649fdff22",
    "8268436f8c4126196cf64b3c7ddbda90746a378625f9813dd9b8457077256731",
    "2810e5cbc2cc4d4eece54f61c6f69758e289aa7ab440b3cbeaa21995c2f4232b",
]


def vote_msgs(rng: random.Random):
    """CanonicalVote sign-bytes of the three sizes the commit path produces."""
    out = []
    for h, chain, rnd, nil in [(1000, "cmtverify-bench", 0, False), (7, "c" * 50, 3, False), (9, "x", 0, True)]:
        bid = None if nil else (hashlib.sha256(b"block%d" % h).digest(), 1, hashlib.sha256(b"parts%d" % h).digest())
        out.append(SB.vote_sign_bytes(chain, 2, h, rnd, bid, 1672531200 + h, rng.randrange(10**9)))
    return out


def alternative_encodings(xs):
    """[(rule, e, log)]: 32-byte strings e the strict decoder rejects and the
    decoder without `rule` (alone) maps into the coset of [log]B, for log = x
    or -x, x in xs; log = 0 stands for the identity's coset E[4]."""
    out = []
    inv = lambda v: pow(v, P - 2, P)  # noqa: E731

    def keep(rule, v, x):
        e = v.to_bytes(32, "little")
        pt = S.ristretto_decode_lenient(e, (rule,))
        if S.ristretto_decode(e) is not None or pt is None:
            return False
        for log in (x, (L - x) % L):  # 1/s lands in the coset of -[x]B
            if S.ristretto_equal(pt, S.scalar_mult(log, S.B)):
                out.append((rule, e, log))
                return True
        return False

    # non-canonical s + p, s < 19: only those that land in E[4] have a known log
    for s in range(0, 19):
        keep("canonical", s + P, 0)
    keep("nonzero_y", P - 1, 0)  # s = -1: canonical, even, square, t = 0, y = 0, order 4
    for x in xs:
        c = int.from_bytes(S.ristretto_encode(S.scalar_mult(x, S.B)), "little")
        assert keep("canonical", c | (1 << 255), x)  # bit 255 set
        assert keep("nonneg_s", P - c, x)            # negative
        # the coset's other representatives: 1/s, -1/s and those times sqrt(-1)
        found = 0
        for v in (inv(c), -inv(c), c * S.SQRT_M1, -c * S.SQRT_M1, inv(c) * S.SQRT_M1, -inv(c) * S.SQRT_M1):
            v %= P
            if v & 1 == 0:  # the odd ones break nonneg_s as well: not discriminating
                found += keep("nonneg_t", v, x)
        assert found, x
    return out


def was_square_search(rng):
    """Whether any non-square encoding is accepted by a verifier without the
    was_square rule, under the two signatures that need no discrete log: the
    identity-style one (s = r, R = [r]B) for the key, and s = k a for R."""
    cands = [v.to_bytes(32, "little") for v in range(0, 1000, 2)] + [bytes.fromhex(h) for h in RFC_BAD]
    cands = [e for e in cands if S.ristretto_decode_lenient(e, ()) is None
             and S.ristretto_decode_lenient(e, ("was_square",)) is not None]
    hits = []
    mini = bytes(range(32))
    a, _ = S.expand_mini(mini)
    pk = S.pubkey_from_mini(mini)
    for e in cands:
        r = rng.randrange(1, L)
        Rb = S.ristretto_encode(S.scalar_mult(r, S.B))
        if S.verify_lenient(e, b"m", S.sign_encoded(0, r, b"m", e, Rb), skip_pk=("was_square",)):
            hits.append(("pk", e.hex()))
        if S.verify_lenient(pk, b"m", S.sign_encoded(a, 0, b"m", pk, e), skip_r=("was_square",)):
            hits.append(("r", e.hex()))
    return len(cands), hits


def lenient_decode_vectors(minis, msgs):
    """The decode_pk / decode_r vectors: for every alternative encoding e of a
    point with a known log, a signature whose transcript runs over e. Key: the
    signer of A = [a]B presents e, R = [r]B, s = r + k a. R: the signature
    carries e_R for R = [r]B. Each dict also names the rule and carries no
    verdict yet."""
    rng = random.Random(SEED + 1)
    scal = [S.expand_mini(m)[0] for m in minis[:3]]
    alts = alternative_encodings(scal)
    # a CanonicalVote, the lengths around the STROBE block end (R = 166), short and long
    pick = [msgs[0]] + [m for m in msgs if len(m) in (165, 166, 167, 0, 300)]
    assert {165, 166, 167} <= {len(m) for m in pick}
    out = []
    for j, (rule, e, x) in enumerate(alts):
        for where, t in (("pk", 0), ("r", 0), ("pk", 1), ("r", 1)):
            m = pick[(2 * j + t + 3 * (where == "r")) % len(pick)]
            other = rng.randrange(1, L)  # the honest side's scalar
            if where == "pk":
                pkb, a, r = e, x, other
                Rb = S.ristretto_encode(S.scalar_mult(r, S.B))
            else:
                a, r, Rb = other, x, e
                pkb = S.ristretto_encode(S.scalar_mult(a, S.B))
            out.append({"cat": "decode_" + where, "rule": rule, "pk": pkb.hex(), "msg": m.hex(),
                        "sig": S.sign_encoded(a, r, m, pkb, Rb).hex()})
    return out


def lenient_verdict(v) -> bool:
    """The verdict of the verifier without v's rule on v's side (decode_pk /
    decode_r vectors)."""
    skip = {"skip_pk" if v["cat"] == "decode_pk" else "skip_r": (v["rule"],)}
    return S.verify_lenient(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"]), **skip)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "sr25519_corpus.json"))
    args = ap.parse_args()
    rng = random.Random(SEED)
    vecs = []

    def add(cat, pk, msg, sig):
        vecs.append({"cat": cat, "pk": bytes(pk).hex(), "msg": bytes(msg).hex(), "sig": bytes(sig).hex()})

    minis = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(24)]
    pks = [S.pubkey_from_mini(m) for m in minis]
    msgs = vote_msgs(rng) + [bytes(rng.randrange(256) for _ in range(n)) for n in
                             [0, 1, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 160, 165, 166, 167, 200, 255, 256, 300]]
    honest = []
    for i, m in enumerate(msgs):
        for j in range(3):
            k = (i * 3 + j) % len(minis)
            sig = S.sign(minis[k], m, nonce_seed=bytes([j]))
            honest.append((pks[k], m, sig))
            add("honest", pks[k], m, sig)
    for pk, m, sig in honest[:40]:
        b = rng.randrange(64 * 8 + max(len(m), 1) * 8)
        s2, m2 = bytearray(sig), bytearray(m)
        if b < 512:
            s2[b // 8] ^= 1 << (b % 8)
        elif m2:
            b -= 512
            m2[b // 8 % len(m2)] ^= 1 << (b % 8)
        else:
            s2[0] ^= 2
        add("bitflip", pk, m2, s2)
    for pk, m, sig in honest[:12]:
        s2 = bytearray(sig)
        s2[63] &= 0x7F
        add("no_marker", pk, m, s2)
    for pk, m, sig in honest[:12]:
        s = int.from_bytes(sig[32:63] + bytes([sig[63] & 0x7F]), "little")
        for s_bad in (s + L, L, 2**255 - 1, L + 1, 2**253):
            sb = bytearray(s_bad.to_bytes(32, "little"))
            sb[31] |= 0x80
            add("s_range", pk, m, sig[:32] + bytes(sb))
    # encodings of public keys and R
    enc_cases = []
    for pk in pks[:8]:
        v = int.from_bytes(pk, "little")
        if v + P < 2**256:
            enc_cases.append(((v + P) % 2**256).to_bytes(32, "little"))  # non-canonical
        enc_cases.append((v | (1 << 255)).to_bytes(32, "little"))        # bit 255
        enc_cases.append((P - v).to_bytes(32, "little"))                 # negative (odd)
    for _ in range(16):  # random even canonical values: mostly non-square / invalid
        v = rng.randrange(P) & ~1
        enc_cases.append(v.to_bytes(32, "little"))
    enc_cases += [bytes.fromhex(h) for h in RFC_BAD]
    for j, e in enumerate(enc_cases):
        pk, m, sig = honest[j % len(honest)]
        add("pk_encoding" if j < len(enc_cases) - len(RFC_BAD) else "rfc_bad", e, m, sig)
        add("r_encoding" if j < len(enc_cases) - len(RFC_BAD) else "rfc_bad", pk, m, e + sig[32:])
    # the identity key: R' = [s]B, valid with s = r
    for i in range(4):
        m = msgs[i]
        r = rng.randrange(1, L)
        Rb = S.ristretto_encode(S.scalar_mult(r, S.B))
        sb = bytearray(r.to_bytes(32, "little"))
        sb[31] |= 0x80
        add("identity_pk", bytes(32), m, Rb + bytes(sb))
    for _ in range(16):
        add("random", bytes(rng.randrange(256) for _ in range(32)), msgs[rng.randrange(len(msgs))],
            bytes(rng.randrange(256) for _ in range(64)))
    vecs += lenient_decode_vectors(minis, msgs)

    # verdicts: Python restatement, cross-checked against the C restatement
    for v in vecs:
        v["valid"] = int(S.verify(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])))
        if "rule" in v:  # discriminating: the strict verdict and the one without the rule differ
            assert v["valid"] == 0 and lenient_verdict(v), v
    pinned = {(v["cat"], v["rule"]) for v in vecs if "rule" in v}
    assert pinned == {(c, r) for c in ("decode_pk", "decode_r") for r in PINNED_RULES}, pinned
    n_nonsquare, hits = was_square_search(random.Random(SEED + 2))
    print("was_square_search:", n_nonsquare, "non-square candidates,", len(hits), "accepted")
    assert n_nonsquare >= 64 and not hits, hits
    assert len(vecs) % 64 != 0  # the GPU tests' last bitmap word stays ragged
    pk = np.array([np.frombuffer(bytes.fromhex(v["pk"]), np.uint8) for v in vecs])
    sig = np.array([np.frombuffer(bytes.fromhex(v["sig"]), np.uint8) for v in vecs])
    m, off = C.pack_msgs([bytes.fromhex(v["msg"]) for v in vecs])
    cv = C.sr25519_verify_batch(pk, sig, m, off)
    bad = [i for i, v in enumerate(vecs) if v["valid"] != int(cv[i])]
    assert not bad, ("C and Python restatements disagree", bad[:10])

    summary = {}
    for v in vecs:
        s = summary.setdefault(v["cat"], {"n": 0, "valid": 0})
        s["n"] += 1
        s["valid"] += v["valid"]
    doc = {
        "generator": "tests/golden/make_sr25519_corpus.py (oracle/sr25519_ref.py)",
        "pins": {"ristretto255_multiples": RISTRETTO_MULTIPLES, "merlin_simple": MERLIN_SIMPLE,
                 "schnorrkel_vector": SCHNORRKEL_VECTOR},
        "summary": summary,
        "vectors": vecs,
    }
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
