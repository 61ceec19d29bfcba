"""Case sets and Python-integer references for tests/dev/devcheck.hip.

Every check_* function builds its cases, runs devcheck once through `run`
(devcases.runner), decodes the raw words and compares them, exactly, with
arbitrary-precision arithmetic (points: oracle/ed25519_ref.py). The lane
checks (LANE_CHECKS) run both on the GPU (tests/test_device_primitives_gpu.py)
and through the DEVCHECK_HOST build (tests/test_device_primitives_host.py),
which is what shows the generators and references right before a GPU is
involved; the row and quad checks need the device's lane exchanges. The
lane checks end with the verdicts' rejection rules (ristretto_decode,
secp_parse_pubkey, secp_sig_scalars, secp_x_is_r and the point formulas)
against oracle/sr25519_ref.py and tests/secp256k1_ref.py.

Where the operand bounds come from:
  MUL_BOUND, SQ_ODD_BOUND   fe25519.h (19 g_i / 38 f_i must fit 32 bits)
  676999 (< 2^19.37)        row.h "Bounds", tests/host/rowcheck.cpp mul_selftest
  0x10000 + 128             row.h "carried" limbs; the bound rowcheck asserts
"""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np

from oracle import ed25519_ref as E
from oracle import sr25519_ref
from tests import secp256k1_ref

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
SQRT_M1 = pow(2, (P - 1) // 4, P)
M26, M25 = 2**26 - 1, 2**25 - 1
MUL_BOUND = 226000000      # fe25519.h
SQ_ODD_BOUND = 113000000   # fe25519.h
ROW_BOUND = 677000         # row.h: inputs below 2^19.37 (rowcheck's limit)
ROW_CARRIED = 0x10000 + 128
SH = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]  # ceil(25.5 i)
P2 = [0x7FFFFDA] + [0x3FFFFFE if i & 1 else 0x7FFFFFE for i in range(1, 10)]  # 2p, limb-wise


def runner(binary):
    """run(op, records[n, IN] u32, blob) -> u32[n, OUT]: one child process,
    never retried; a non-zero exit, a fault or the time limit raises."""
    def run(op, recs, blob=b""):
        recs = np.ascontiguousarray(recs, dtype=np.uint32)
        n = recs.shape[0]
        buf = struct.pack("<II", n, len(blob)) + recs.tobytes() + blob
        out = subprocess.run([binary, op], input=buf, capture_output=True, timeout=60, check=True).stdout
        a = np.frombuffer(out, np.uint32)
        assert a.size and a.size % n == 0, (op, n, a.size)
        return a.reshape(n, -1)
    return run


def words(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def unwords(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


# ---- radix 2^25.5 -------------------------------------------------------------------

def fe_val(limbs):
    return sum(int(x) << s for x, s in zip(limbs, SH))


def fe_limbs(v):
    """v < 2^256 in canonical-width limbs (limb 9 takes what is above 2^255)"""
    return [(v >> SH[i]) & (M25 if i & 1 else M26) for i in range(9)] + [v >> 230]


def fe_loose(limbs):
    """the same value mod p: 2p added limb-wise, and one unit of every limb
    above 0 moved down to its neighbour"""
    out = [a + b for a, b in zip(limbs, P2)]
    for i in range(1, 10):
        if out[i] > 0:
            out[i] -= 1
            out[i - 1] += 1 << (SH[i] - SH[i - 1])
    return out


def reduce64_excess():
    """How far limbs 1 and 5 of a product may exceed 2^25 - 1 ("odd limbs
    < 2^25 (+tiny)", fe25519.h). fe_reduce64 runs two interleaved carry
    streams (0 -> 4 and 4 -> 9) and then two more steps, and the limb that
    receives a stream's last carry is not carried again:
      limb 1: the carry out of limb 9 is folded into limb 0 (x 19), and limb
              0's carry then lands on the already masked limb 1;
      limb 5: the first stream ends with a second carry out of limb 4 (masked
              limb 4 plus limb 3's carry), which lands on the masked limb 5.
    Every other limb is masked after its last addition. Upper bounds by
    running the chain on the largest column sums (every limb of both operands
    at MUL_BOUND - 1): a carry floor(h / 2^k) is monotone in h, and a masked
    limb is at most its mask."""
    b = MUL_BOUND - 1
    h = [0] * 10
    for i in range(10):
        for j in range(10):
            h[(i + j) % 10] += (2 if i & 1 and j & 1 else 1) * (19 if i + j >= 10 else 1) * b * b
    assert max(h) == 267 * b * b < 2**64  # fe25519.h: the worst column fits 64 bits
    for i, bits in ((0, 26), (4, 26), (1, 25), (5, 25), (2, 26), (6, 26), (3, 25), (7, 25), (4, 26), (8, 26)):
        h[i + 1] += h[i] >> bits
        assert h[i + 1] < 2**64
        h[i] = (1 << bits) - 1
    h[0] += 19 * (h[9] >> 25)
    return {1: h[0] >> 26, 5: h[5] - M25}


PRODUCT_EXCESS = reduce64_excess()


def assert_carried(limbs, what, excess=PRODUCT_EXCESS):
    for i, x in enumerate(limbs):
        lim = M25 if i & 1 else M26
        assert int(x) <= lim + excess.get(i, 0), (what, i, int(x))


def _rand_limbs(rng, bounds):
    return [int(rng.integers(0, b)) for b in bounds]


def product_cases(rng, sq=False):
    """(f, g) raw-limb pairs of the classes the issue lists; a multiple of 64,
    every lane different. sq: odd limbs stay below SQ_ODD_BOUND."""
    bd = [SQ_ODD_BOUND if (sq and i & 1) else MUL_BOUND for i in range(10)]
    top = [b - 1 for b in bd]
    carried = [M25 if i & 1 else M26 for i in range(10)]
    submax = [3 * 2**25 if i & 1 else 3 * 2**26 for i in range(10)]
    cases = [(top, top), (carried, carried), (submax, submax), (top, carried), (submax, top)]
    for i in range(10):  # one limb at the bound, the rest zero, on either operand
        one = [top[i] if j == i else 0 for j in range(10)]
        cases += [(one, _rand_limbs(rng, bd)), (_rand_limbs(rng, bd), one), (one, top)]
    for ph in (0, 1):    # alternating bound and zero
        alt = [top[j] if (j & 1) == ph else 0 for j in range(10)]
        cases += [(alt, alt), (alt, top), (top, alt)]
    while len(cases) % 64 or len(cases) < 256:
        if len(cases) & 1:
            cases.append((_rand_limbs(rng, bd), _rand_limbs(rng, bd)))
        else:
            cases.append((_rand_limbs(rng, [c + 1 for c in carried]), _rand_limbs(rng, [c + 1 for c in carried])))
    return cases


def _check_products(out, want, what):
    for j, (row, w) in enumerate(zip(out.tolist(), want)):
        assert fe_val(row) % P == w, (what, j)
        assert_carried(row, (what, j))


def check_fe_mul(run):
    cases = product_cases(np.random.default_rng(1))
    out = run("fe_mul", [f + g for f, g in cases])
    _check_products(out, [fe_val(f) * fe_val(g) % P for f, g in cases], "fe_mul")


def check_fe_sq(run):
    cases = product_cases(np.random.default_rng(2), sq=True)
    out = run("fe_sq", [f for f, _ in cases])
    _check_products(out, [pow(fe_val(f), 2, P) for f, _ in cases], "fe_sq")


def check_fe_sqn(run, n):
    cases = product_cases(np.random.default_rng(3 + n), sq=True)
    out = run(f"fe_sqn{n}", [g for _, g in cases])
    _check_products(out, [pow(fe_val(g), 2**n, P) for _, g in cases], f"fe_sqn{n}")


def check_fe_carry(run):
    """Inputs up to 2^31 - 1 per limb: with every limb below 2^31 a carry is
    below 2^6 and 19 c below 2^11, so no limb's sum leaves 32 bits. After the
    last step limb 0 was below 2^26 + 19 * 2^6, so limb 1 exceeds 2^25 - 1 by
    at most 1."""
    rng = np.random.default_rng(4)
    top = [2**31 - 1] * 10
    cases = [top, [0] * 10, P2, [3 * 2**25 if i & 1 else 3 * 2**26 for i in range(10)]]
    cases += [[top[j] if j == i else 0 for j in range(10)] for i in range(10)]
    while len(cases) % 64:
        cases.append(_rand_limbs(rng, [2**31] * 10))
    out = run("fe_carry", cases)
    for j, (row, f) in enumerate(zip(out.tolist(), cases)):
        assert fe_val(row) % P == fe_val(f) % P, j
        assert_carried(row, ("fe_carry", j), excess={1: 1})


def check_fe_lin(run):
    """fe_add / fe_sub / fe_neg feeding a product: (f + g) k, (f - g) k, (-g) k
    with f, g carried (fe_sub's stated operands) and k up to MUL_BOUND - 1. f
    at the carried maximum and g = 0 gives fe_sub's largest limbs (3 * 2^26 /
    3 * 2^25 less a little), g at the maximum its smallest."""
    rng = np.random.default_rng(5)
    cmax = [M25 if i & 1 else M26 for i in range(10)]
    zero = [0] * 10
    top = [MUL_BOUND - 1] * 10
    cases = [(cmax, zero, top), (cmax, cmax, top), (zero, cmax, top), (zero, zero, top), (cmax, zero, cmax)]
    while len(cases) % 64:
        cases.append((_rand_limbs(rng, [c + 1 for c in cmax]), _rand_limbs(rng, [c + 1 for c in cmax]),
                      _rand_limbs(rng, [MUL_BOUND] * 10)))
    out = run("fe_lin", [f + g + k for f, g, k in cases]).tolist()
    for j, (f, g, k) in enumerate(cases):
        a, b, c = fe_val(f), fe_val(g), fe_val(k)
        for part, w in enumerate(((a + b) * c % P, (a - b) * c % P, -b * c % P)):
            row = out[j][10 * part: 10 * part + 10]
            assert fe_val(row) % P == w, (j, part)
            assert_carried(row, ("fe_lin", j, part))


def check_fe_frombytes(run):
    rng = np.random.default_rng(6)
    vals = [2**256 - 1, 2**255, 2**255 - 1, 0, 1, P, P - 1, 2**255 + P, 2**255 + 1]
    while len(vals) % 64:
        vals.append(int.from_bytes(rng.bytes(32), "little"))
    out = run("fe_frombytes", [words(v, 8) for v in vals]).tolist()
    for j, v in enumerate(vals):
        assert out[j] == fe_limbs(v & (2**255 - 1)), j  # bit 255 ignored, the value not reduced


def canon_values():
    return [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1] + [2**255 - k for k in range(20, 0, -1)] + [SQRT_M1]


def check_fe_canon(run):
    """fe_tobytes / fe_iszero / fe_isneg on the edge values, each in
    canonical-width limbs and in a loose representation of the same value."""
    rng = np.random.default_rng(7)
    vals = canon_values()
    cases = [(v, fe_limbs(v)) for v in vals] + [(v, fe_loose(fe_limbs(v))) for v in vals]
    cases += [(v, fe_loose(fe_loose(fe_limbs(v)))) for v in vals]
    while len(cases) % 64:
        v = int.from_bytes(rng.bytes(32), "little")
        cases.append((v, fe_loose(fe_limbs(v)) if len(cases) & 1 else fe_limbs(v)))
    assert all(fe_val(l) % P == v % P and max(l) < 2**32 for v, l in cases)
    out = run("fe_canon", [l for _, l in cases]).tolist()
    for j, (v, _) in enumerate(cases):
        c = v % P
        assert unwords(out[j][:8]) == c, j
        assert out[j][8] == (c == 0) and out[j][9] == (c & 1), j


def check_fe_equal(run):
    rng = np.random.default_rng(8)
    cases = []
    for v in canon_values():
        a = fe_limbs(v)
        cases += [(a, fe_loose(a), 1), (a, fe_limbs((v + 1) % 2**255), (v + 1) % 2**255 % P == v % P),
                  (fe_loose(a), fe_limbs(v % P), 1)]
    while len(cases) % 64:
        v, w = (int.from_bytes(rng.bytes(32), "little") >> 1 for _ in range(2))
        cases.append((fe_limbs(v), fe_limbs(w), v % P == w % P))
    out = run("fe_equal", [a + b for a, b, _ in cases]).tolist()
    for j, (a, b, w) in enumerate(cases):
        assert out[j][0] == int(w), j


def check_fe_pow(run):
    rng = np.random.default_rng(9)
    cases = [fe_limbs(v) for v in (0, 1, P - 1, SQRT_M1, 2, P - 2)]
    cases.append([(SQ_ODD_BOUND if i & 1 else MUL_BOUND) - 1 for i in range(10)])  # fe_sq's input bound
    cases.append([M25 if i & 1 else M26 for i in range(10)])
    while len(cases) % 64:
        cases.append(fe_limbs(int.from_bytes(rng.bytes(32), "little") >> 1))
    out = run("fe_pow", cases).tolist()
    for j, l in enumerate(cases):
        z = fe_val(l) % P
        assert fe_val(out[j][:10]) % P == pow(z, P - 2, P), j
        assert fe_val(out[j][10:]) % P == pow(z, (P - 5) // 8, P), j
        assert_carried(out[j][:10], ("invert", j))
        assert_carried(out[j][10:], ("pow22523", j))


# ---- scalars and hashes ---------------------------------------------------------------

def check_sc_reduce512(run):
    rng = np.random.default_rng(10)
    m = (2**512 - 1) // L * L
    vals = [0, L - 1, L, L + 1, 2**252, 2**256 - 1, 2**512 - 1, m, m - 1, m + 1, 2**252 - 1, 2 * L, 2 * L - 1]
    while len(vals) % 64:
        vals.append(int.from_bytes(rng.bytes(64), "little"))
    out = run("sc_reduce512", [words(v, 16) for v in vals]).tolist()
    for j, v in enumerate(vals):
        assert unwords(out[j]) == v % L, j


def check_sc_is_canonical(run):
    rng = np.random.default_rng(11)
    vals = [L - 1, L, L + 1, 0, 2**255, 2**254, 2**253, 2**255 + 5, 2**254 + L - 1, 2**253 - 1, 2**252, 2**256 - 1]
    while len(vals) % 64:
        vals.append(int.from_bytes(rng.bytes(32), "little") >> int(rng.integers(0, 5)))
    out = run("sc_is_canonical", [words(v, 8) for v in vals]).tolist()
    for j, v in enumerate(vals):
        assert out[j][0] == int(v < L), j


def check_sc_muladd(run):
    rng = np.random.default_rng(12)
    cases = [(L - 1, L - 1, L - 1), (0, 0, 0), (1, L - 1, 1), (2**256 - 1, 2**256 - 1, 2**256 - 1)]
    while len(cases) % 64:
        cases.append(tuple(int.from_bytes(rng.bytes(32), "little") % L for _ in range(3)))
    out = run("sc_muladd", [words(a, 8) + words(b, 8) + words(c, 8) for a, b, c in cases]).tolist()
    for j, (a, b, c) in enumerate(cases):
        assert unwords(out[j]) == (a * b + c) % L, j


def half_scalars_cases():
    """the first 4,096 scalars of test_host_math.test_half_scalar_decomposition
    (its boundary values included), shuffled so that wide, 34-window and
    ordinary scalars share waves"""
    rng = np.random.default_rng(215)
    ks = [0, 1, 2, 3, L - 1, L - 2, 2**127, 2**128 - 1, 2**134, 2**252]
    ks += [int.from_bytes(rng.bytes(32), "little") % L for _ in range(20000)]
    ks = ks[:4096]
    order = np.random.default_rng(216).permutation(len(ks))
    return [ks[i] for i in order]


def halfcheck_reference(ks, odd):
    """tests/host/halfcheck.cpp's records (k1 | k2 | flags, the Lehmer run)"""
    from tests.host import hostbuild

    binary = hostbuild.build(os.path.join(ROOT, "tests", "host", "halfcheck.cpp"),
                             os.path.join(ROOT, "build", "halfcheck"), ["-std=c++17"])
    buf = struct.pack("<I", len(ks)) + b"".join(k.to_bytes(32, "little") for k in ks)
    out = subprocess.run([binary, "odd" if odd else "any"], input=buf, capture_output=True, check=True,
                         timeout=120).stdout
    assert len(out) == 130 * len(ks)
    return [out[130 * j: 130 * j + 65] for j in range(len(ks))]


def _half_records(row):
    return np.asarray(row[:16], np.uint32).tobytes() + bytes([row[16]])


def check_half(run, odd, uni=False):
    ks = half_scalars_cases()
    want = halfcheck_reference(ks, odd)
    out = run("half_uni" if uni else "half", [words(k, 8) + [int(odd)] for k in ks]).tolist()
    for j in range(len(ks)):
        assert out[j][16] < 256 and _half_records(out[j]) == want[j], j
        if uni:
            assert out[j][17] == 1, j  # all 64 lanes of the wave agree
    # the case set holds wide scalars and, with k2 odd, 34-window pairs
    assert any(w[64] & 2 for w in want) and (not odd or any((w[64] >> 2) == 2 for w in want))


def check_hs_prims(run):
    """hs_udiv31 (the device divides in double precision) is floor(a / b) for
    0 <= a < 2^31, 0 < b < 2^31, also where a / b is one below or exactly an
    integer; hs_clz on every bit position and on 0. The decomposition's
    output cannot show a wrong quotient here: Lehmer's corner check rejects it
    and the exact Euclid steps take over (slower, the same pair)."""
    rng = np.random.default_rng(17)
    top = 2**31 - 1
    cases = [(0, 1, 0), (top, 1, 1), (top, top, top), (top - 1, top, 2**31), (top, 2, 2**32 - 1), (1, top, 3)]
    cases += [(0, top, 1 << i) for i in range(32)]
    while len(cases) % 64 or len(cases) < 1024:
        b = int(rng.integers(1, 2 ** int(rng.integers(1, 32))))
        q = int(rng.integers(0, top // b + 1))
        a = min(top, max(0, q * b + int(rng.integers(-1, 2))))  # q b - 1, q b, q b + 1
        cases.append((a, b, int(rng.integers(0, 2**32)) >> int(rng.integers(0, 32))))
    out = run("hs_prims", cases).tolist()
    for j, (a, b, x) in enumerate(cases):
        assert out[j] == [a // b, 32 - x.bit_length()], (j, a, b, x)


def check_sha512(run, pw):
    """every length 0..400 at each of the four alignments of the message
    pointer, one lane per case, shuffled so trip counts diverge in a wave"""
    rng = np.random.default_rng(13 + pw)
    cases = [(n, a) for n in range(401) for a in range(4)]
    cases = [cases[i] for i in rng.permutation(len(cases))]
    blob = bytearray()
    recs, want = [], []
    for n, a in cases:
        blob += rng.bytes(4 + (a - len(blob)) % 4)  # random filler up to the alignment
        off = len(blob)
        assert off % 4 == a
        msg = rng.bytes(n)
        blob += msg
        pre = rng.integers(0, 2**32, pw, dtype=np.uint32)
        recs.append([off, n] + pre.tolist())
        want.append(hashlib.sha512(pre.tobytes() + msg).digest())
    blob += rng.bytes(7)
    out = run(f"sha512_{pw}", recs, bytes(blob))
    for j in range(len(cases)):
        assert out[j].tobytes() == want[j], (j, cases[j])


def check_keccak(run):
    rng = np.random.default_rng(14)
    states = [bytes(200), b"\xff" * 200] + [rng.bytes(200) for _ in range(62)]
    out = run("keccak", [np.frombuffer(s, np.uint32) for s in states])
    for j, s in enumerate(states):
        st = bytearray(s)
        sr25519_ref.keccak_f1600(st)
        assert out[j].tobytes() == bytes(st), j


# ---- the verdicts' rejection rules (sr25519.h, secp256k1.h) ---------------------------------
# One record per lane, whole waves of different inputs; verdicts and values
# compared exactly with oracle/sr25519_ref.py and tests/secp256k1_ref.py.

def _sr_corpus_encodings():
    """every key and R of the sr25519 corpus's encoding categories: all of the
    generator's RFC_BAD, the decode_pk / decode_r alternative encodings, the
    non-canonical / negative / random ones of pk_encoding / r_encoding"""
    with open(os.path.join(ROOT, "tests", "golden", "sr25519_corpus.json")) as f:
        vecs = json.load(f)["vectors"]
    cats = {"rfc_bad", "decode_pk", "decode_r", "pk_encoding", "r_encoding"}
    encs = []
    for v in vecs:
        if v["cat"] in cats:
            for e in (bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"])[:32]):
                if e not in encs:
                    encs.append(e)
    return encs


def check_ristretto_decode(run):
    """ristretto_decode's verdict on every input, its point where the strict
    oracle accepts. The case set holds, for each of the five rules, encodings
    that break that rule alone (asserted): this is what pins was_square, which
    no signature can reach (tests/golden/make_sr25519_corpus.py)."""
    S = sr25519_ref
    rng = np.random.default_rng(60)
    encs = _sr_corpus_encodings()
    encs += [v.to_bytes(32, "little") for v in (0, P - 1, P, P + 1, 2**255 - 1, 2**255, 2**256 - 1, 1, 2, P - 2)]
    mult = [S.ristretto_encode(S.scalar_mult(k, S.B)) for k in range(1, 17)]
    encs += mult + [(int.from_bytes(e, "little") | 1 << 255).to_bytes(32, "little") for e in mult[:4]]
    while len(encs) % 64 or len(encs) < 320:
        encs.append((int.from_bytes(rng.bytes(32), "little") % P & ~1).to_bytes(32, "little"))  # about 1 in 8 decodes
    out = run("ristretto_decode", [np.frombuffer(e, np.uint32) for e in encs]).tolist()
    alone = set()
    for j, e in enumerate(encs):
        pt = S.ristretto_decode(e)
        assert out[j][0] == int(pt is not None), (j, e.hex())
        if pt is not None:
            got = tuple(unwords(out[j][1 + 8 * c: 9 + 8 * c]) for c in range(3))
            assert got == (pt[0], pt[1], pt[3]), (j, e.hex())
        else:
            broken = [r for r in S.DECODE_RULES
                      if S.ristretto_decode_lenient(e, tuple(set(S.DECODE_RULES) - {r})) is None]
            if len(broken) == 1:
                alone.add(broken[0])
    assert alone == set(S.DECODE_RULES), alone
    assert sum(o[0] for o in out) >= 32


def check_sqrt_ratio_m1(run):
    """fe_sqrt_ratio_m1 against RFC 9496's SQRT_RATIO_M1: u / v square, i u / v
    square, u = 0, v = 0, both; u, v carried (canonical-width limbs)"""
    rng = np.random.default_rng(61)

    def rnd():
        return int.from_bytes(rng.bytes(32), "little") % P or 1

    cases = [(0, 0), (0, 1), (1, 0), (1, 1), (P - 1, 1), (1, P - 1), (SQRT_M1, 1), (P - SQRT_M1, 1), (4, 1), (1, 4),
             (2**255 - 20, 2**255 - 20), (2, 1), (1, 2)]
    while len(cases) % 64 or len(cases) < 256:
        r0, v = rnd(), rnd()
        k = len(cases) % 4
        cases.append([(r0 * r0 * v % P, v), (SQRT_M1 * r0 * r0 * v % P, v), (0, v), (r0, 0)][k])
    out = run("sqrt_ratio_m1", [fe_limbs(u) + fe_limbs(v) for u, v in cases]).tolist()
    seen = set()
    for j, (u, v) in enumerate(cases):
        sq, r = sr25519_ref.sqrt_ratio_m1(u, v)
        assert out[j][0] == int(sq) and unwords(out[j][1:]) == r, (j, u, v)
        assert r & 1 == 0 and (v * r * r - (u if sq else SQRT_M1 * u)) % P == 0 or v == 0, j  # the definition
        seen.add((bool(sq), u == 0, v == 0))
    assert seen >= {(True, False, False), (False, False, False), (True, True, False), (False, False, True),
                    (True, True, True)}  # (was_square, u = 0, v = 0)


K = secp256k1_ref
FP_P = K.P
FP_M26, FP_M22 = 2**26 - 1, 2**22 - 1
FP_P_LIMBS = [0x3FFFC2F, 0x3FFFFBF] + [FP_M26] * 7 + [FP_M22]


def fp_limbs(v):
    assert 0 <= v < 2**256
    return [(v >> (26 * i)) & FP_M26 for i in range(9)] + [v >> 234]


def fp_val(limbs):
    return sum(int(x) << (26 * i) for i, x in enumerate(limbs))


def fp_mag(v, m):
    """v mod p at magnitude m (fp256k1.h): canonical limbs plus (2 m - 1) p
    limb-wise, every limb between (2 m - 1) / (2 m) of its bound and the bound"""
    out = [a + (2 * m - 1) * b for a, b in zip(fp_limbs(v % FP_P), FP_P_LIMBS)]
    assert fp_within(out, m) and not fp_within(out, m - 1) and fp_val(out) % FP_P == v % FP_P
    return out


def fp_within(limbs, m):
    return all(int(x) <= 2 * m * FP_M26 for x in limbs[:9]) and int(limbs[9]) <= 2 * m * FP_M22


def check_secp_parse_pubkey(run):
    """secp_parse_pubkey: every prefix, x at and around p (never reduced), x + p
    for small x on the curve, x off the curve, both parities"""
    rng = np.random.default_rng(62)
    on = [x for x in range(1, 40) if K.lift_x(x, 0) is not None][:6]
    off = [x for x in range(1, 40) if K.lift_x(x, 0) is None][:6]
    assert on and off
    keys = []
    for x in on + off + [FP_P - 1, FP_P, FP_P + 1, 2**256 - 1, 0, K.GX] + [x + FP_P for x in on]:
        for prefix in (2, 3):
            keys.append(bytes([prefix]) + x.to_bytes(32, "big"))
    for prefix in (0, 1, 2, 3, 4, 5, 6, 7, 0xFF, 0x82, 0x12):
        keys.append(bytes([prefix]) + K.GX.to_bytes(32, "big"))
    while len(keys) % 64 or len(keys) < 256:
        k = len(keys) % 8
        x = int.from_bytes(rng.bytes(32), "big")
        if k == 7:
            x |= (2**256 - 2**33)  # x >= p about half of the time
        keys.append(bytes([(2, 3, 2, 3, 3, 2, int(rng.integers(0, 256)), 2)[k]]) + x.to_bytes(32, "big"))
    out = run("secp_parse_pubkey", [np.frombuffer(k + b"\0\0\0", np.uint32) for k in keys]).tolist()
    seen = set()
    for j, k in enumerate(keys):
        q = K.parse_pubkey(k)
        assert out[j][0] == int(q is not None), (j, k.hex())
        if q is not None:
            assert (unwords(out[j][1:9]), unwords(out[j][9:17])) == (q[0], q[1]), (j, k.hex())
            seen.add(q[1] & 1)
    assert seen == {0, 1} and 32 <= sum(o[0] for o in out) <= len(keys) - 32
    # x + p for x on the curve is rejected only by x < p
    assert all(K.parse_pubkey(bytes([2]) + (x + FP_P).to_bytes(32, "big")) is None for x in on)


def check_secp_sig_scalars(run):
    """secp_sig_scalars: r and s reduced mod n; false for r = 0, s = 0 (also as
    the bytes of n) and s above (n - 1) / 2"""
    rng = np.random.default_rng(63)
    n = K.N
    edge = [0, 1, n - 1, n, n + 1, (n - 1) // 2, (n + 1) // 2, 2**256 - 1]
    cases = [(r, s) for r in edge for s in edge]
    while len(cases) % 64 or len(cases) < 256:
        r, s = (int.from_bytes(rng.bytes(32), "big") for _ in range(2))
        cases.append((r, s >> int(rng.integers(0, 3))))
    recs = [np.frombuffer(r.to_bytes(32, "big") + s.to_bytes(32, "big"), np.uint32) for r, s in cases]
    out = run("secp_sig_scalars", recs).tolist()
    for j, (r, s) in enumerate(cases):
        ok = r % n != 0 and s % n != 0 and s % n <= K.HALF_N
        assert out[j] == [int(ok)] + words(r % n, 8) + words(s % n, 8), (j, hex(r), hex(s))
    # r = 0 alone: everything else about the signature passes
    assert sum(1 for r, s in cases if r % n == 0 and 0 < s % n <= K.HALF_N) >= 6


def _acc(x, z, mags, y=None):
    """the accumulator (x z : y z : z) at magnitudes mags = (mx, my, mz)"""
    y = 1 if y is None else y
    return fp_mag(x * z, mags[0]) + fp_mag(y * z, mags[1]) + fp_mag(z, mags[2])


def check_secp_x_is_r(run):
    """secp_x_is_r on constructed accumulators (x z : y : z), z random,
    canonical limbs and magnitude (3, 2, 2): x = r; x = r + n < p; the two ways
    r + n can leave the field (r + n >= 2^256 with x = r + n - 2^256, and
    p <= r + n < 2^256 with x = r + n - p: both false, only `wraps` says so);
    Z = 0 = X (false, only the Z test says so); x = r + 1"""
    rng = np.random.default_rng(64)
    n, p = K.N, FP_P

    def below(lo, hi):
        return lo + int.from_bytes(rng.bytes(40), "big") % (hi - lo)

    cases = []  # (limbs, r, class)
    for t in range(40):
        mags = (3, 2, 2) if t & 1 else (1, 1, 1)
        z = below(1, p)
        r = [1, p - n - 1, n - 1][t] if t < 3 else below(1, n)
        if r < n - 1:
            cases.append((_acc(r, z, mags), r, "x = r"))
            cases.append((_acc(r + 1, z, mags), r, "x = r + 1"))
        r = [1, p - n - 1][t] if t < 2 else below(1, p - n)
        cases.append((_acc(r + n, z, mags), r, "x = r + n"))
        r = [2**256 - n, n - 1][t] if t < 2 else below(2**256 - n, n)
        cases.append((_acc(r + n - 2**256, z, mags), r, "wraps 2^256"))
        r = [p - n, 2**256 - n - 1][t] if t < 2 else below(p - n, 2**256 - n)
        cases.append((_acc(r + n - p, z, mags), r, "wraps p"))
        r = below(1, n)
        cases.append((fp_mag(0, mags[0]) + fp_mag(below(1, p), mags[1]) + fp_mag(0, mags[2]), r, "infinity"))
        cases.append(([0] * 10 + fp_limbs(1) + [0] * 10, r, "infinity"))
    while len(cases) % 64:
        r = below(1, n)
        cases.append((_acc(below(0, p), below(1, p), (3, 2, 2)), r, "random"))
    out = run("secp_x_is_r", [l + words(r, 8) for l, r, _ in cases]).tolist()
    want_by_class = {"x = r": 1, "x = r + n": 1, "x = r + 1": 0, "wraps 2^256": 0, "wraps p": 0, "infinity": 0}
    for j, (l, r, cls) in enumerate(cases):
        X, Z = fp_val(l[:10]) % p, fp_val(l[20:]) % p
        want = int(Z != 0 and X * pow(Z, p - 2, p) % p % n == r)
        assert want == want_by_class.get(cls, want), (j, cls)
        assert out[j][0] == want, (j, cls, hex(r))
        if cls.startswith("wraps"):  # r + n read as 256 bits and as a field element gives X = that Z
            assert ((r + n) % 2**256 * Z - X) % p == 0, j
    assert {c for _, _, c in cases} >= set(want_by_class)


def _secp_points():
    """affine points: G, 2G, 3G, [n - 1]G, the x = 1 point, random multiples"""
    rng = np.random.default_rng(65)
    pts = [K.to_affine(K.gmul(k)) for k in (1, 2, 3, K.N - 1, K.N - 2)] + [K.lift_x(1, 0)[:2]]
    pts += [K.to_affine(K.gmul(int.from_bytes(rng.bytes(32), "big") % K.N or 1)) for _ in range(26)]
    return pts


def _proj(pt, z, mags, yneg=False):
    """(x z : y z : z) at magnitudes mags; None: infinity (0 : z : 0)"""
    if pt is None:
        return fp_mag(0, mags[0]) + fp_mag(z, mags[1]) + fp_mag(0, mags[2])
    x, y = pt
    return fp_mag(x * z, mags[0]) + fp_mag((-y if yneg else y) * z, mags[1]) + fp_mag(z, mags[2])


def _aff_neg(pt):
    return None if pt is None else (pt[0], -pt[1] % FP_P)


def _check_point_out(row, want, mags, what):
    l = [row[0:10], row[10:20], row[20:30]]
    assert row[30] == 7 and all(fp_within(a, m) for a, m in zip(l, mags)), (what, "magnitude")
    X, Y, Z = (fp_val(a) % FP_P for a in l)
    if want is None:
        assert X == 0 and Z == 0 and Y != 0, (what, "infinity")
    else:
        zi = pow(Z, FP_P - 2, FP_P)
        assert Z != 0 and (X * zi % FP_P, Y * zi % FP_P) == tuple(want), what


def _aff_add(a, b):
    s = K.jadd(None if a is None else (a[0], a[1], 1), None if b is None else (b[0], b[1], 1))
    return None if s is None else K.to_affine(s)


def check_pt_add(run):
    """pt_add (complete, RCB algorithm 7) against affine big-integer addition:
    P + P, P + (-P), infinity on either side and on both, a table entry with Y
    negated at (3, 3, 2), both operands at (3, 3, 2), canonical limbs; the
    output within (3, 2, 2)"""
    rng = np.random.default_rng(66)
    pts = _secp_points()

    def z():
        return int.from_bytes(rng.bytes(32), "big") % FP_P or 1

    tight, acc, entry = (1, 1, 1), (3, 2, 2), (3, 3, 2)
    cases = []  # (p limbs, q limbs, affine sum)
    for i, a in enumerate(pts):
        b = pts[(i + 7) % len(pts)]
        for ma, mb in ((tight, tight), (acc, entry), (entry, entry)):
            cases.append((_proj(a, z(), ma), _proj(a, z(), mb), _aff_add(a, a)))                      # P + P
            cases.append((_proj(a, z(), ma), _proj(a, z(), mb, yneg=True), None))                      # P + (-P)
            cases.append((_proj(a, z(), ma), _proj(b, z(), mb, yneg=True), _aff_add(a, _aff_neg(b))))  # P - Q
            cases.append((_proj(a, z(), ma), _proj(b, z(), mb), _aff_add(a, b)))
        cases.append((_proj(None, z(), acc), _proj(a, z(), entry), a))
        cases.append((_proj(a, z(), acc), _proj(None, z(), entry), a))
        cases.append((_proj(None, z(), acc), _proj(None, z(), entry), None))
        cases.append((_proj(None, 1, tight), _proj(a, 1, tight), a))
    while len(cases) % 64:
        a, b = pts[len(cases) % len(pts)], pts[(3 * len(cases) + 1) % len(pts)]
        cases.append((_proj(a, z(), entry), _proj(b, z(), acc), _aff_add(a, b)))
    out = run("pt_add", [a + b for a, b, _ in cases]).tolist()
    for j, (_, _, want) in enumerate(cases):
        _check_point_out(out[j], want, (3, 2, 2), ("pt_add", j))
    assert sum(1 for c in cases if c[2] is None) >= 64


def check_pt_double(run):
    """pt_double (RCB algorithm 9) against affine doubling: points and
    infinity, canonical limbs and magnitudes (3, 2, 2) and (3, 3, 2); the
    output within (2, 2, 1)"""
    rng = np.random.default_rng(67)
    cases = []
    for a in [None, None] + _secp_points():
        for mags in ((1, 1, 1), (3, 2, 2), (3, 3, 2), (2, 2, 1)):
            zz = int.from_bytes(rng.bytes(32), "big") % FP_P or 1
            cases.append((_proj(a, zz, mags), _aff_add(a, a)))
            cases.append((_proj(a, zz, mags, yneg=True), _aff_add(_aff_neg(a), _aff_neg(a))))
    cases = cases[: len(cases) // 64 * 64]
    assert len(cases) >= 256 and sum(1 for c in cases if c[1] is None) >= 8
    out = run("pt_double", [a for a, _ in cases]).tolist()
    for j, (_, want) in enumerate(cases):
        _check_point_out(out[j], want, (2, 2, 1), ("pt_double", j))


LANE_CHECKS = {
    "fe_mul": check_fe_mul,
    "fe_sq": check_fe_sq,
    "fe_sqn1": lambda run: check_fe_sqn(run, 1),
    "fe_sqn2": lambda run: check_fe_sqn(run, 2),
    "fe_sqn5": lambda run: check_fe_sqn(run, 5),
    "fe_sqn50": lambda run: check_fe_sqn(run, 50),
    "fe_carry": check_fe_carry,
    "fe_add_sub_neg": check_fe_lin,
    "fe_frombytes": check_fe_frombytes,
    "fe_tobytes_iszero_isneg": check_fe_canon,
    "fe_equal": check_fe_equal,
    "fe_invert_pow22523": check_fe_pow,
    "sc_reduce512": check_sc_reduce512,
    "sc_is_canonical": check_sc_is_canonical,
    "sc_muladd": check_sc_muladd,
    "half_scalars_odd": lambda run: check_half(run, True),
    "half_scalars_any": lambda run: check_half(run, False),
    "hs_udiv31_clz": check_hs_prims,
    "sha512_prefixed_16": lambda run: check_sha512(run, 16),
    "sha512_prefixed_8": lambda run: check_sha512(run, 8),
    "keccak_f1600": check_keccak,
    "ristretto_decode": check_ristretto_decode,
    "fe_sqrt_ratio_m1": check_sqrt_ratio_m1,
    "secp_parse_pubkey": check_secp_parse_pubkey,
    "secp_sig_scalars": check_secp_sig_scalars,
    "secp_x_is_r": check_secp_x_is_r,
    "pt_add": check_pt_add,
    "pt_double": check_pt_double,
}


# ---- row layer (DevRow): lane 16 c + k of a wave = limb k of row c ---------------------

def row_val(l):
    return sum(int(x) << (16 * k) for k, x in enumerate(l))


def row_limbs(v):
    return [(v >> (16 * k)) & 0xFFFF for k in range(16)]


def row_cases(rng, trials=200):
    """rowcheck's mul_selftest (limb limits 677000, 0x10000, 0x10600), plus:
    every limb at 676999; one limb at 676999 and the rest zero for each of the
    16 positions on either operand (each wrap-twist column on its own); the
    carried maximum 0x10000 + 128. (f, g) rows; a multiple of 16 (4 waves)."""
    top = [ROW_BOUND - 1] * 16
    cmax = [ROW_CARRIED] * 16
    cases = [(top, top), (cmax, cmax), (top, cmax), (cmax, top)]
    for i in range(16):
        one = [ROW_BOUND - 1 if j == i else 0 for j in range(16)]
        cases += [(one, top), (top, one), (one, [int(x) for x in rng.integers(0, ROW_BOUND, 16)]),
                  ([int(x) for x in rng.integers(0, ROW_BOUND, 16)], one)]
    for lim in (ROW_BOUND, 0x10000, 0x10600):
        for _ in range(trials):
            cases.append(([int(x) for x in rng.integers(0, lim, 16)], [int(x) for x in rng.integers(0, lim, 16)]))
    while len(cases) % 16:
        cases.append(([int(x) for x in rng.integers(0, ROW_BOUND, 16)], [int(x) for x in rng.integers(0, ROW_BOUND, 16)]))
    return cases


def _row_records(cases, share=1):
    """lane records (f, g); share = S: each case on S rows of its wave (S = 2:
    rows c and c ^ 2, S = 4: all four), different cases across groups"""
    rows = []
    if share == 1:
        rows = cases
    elif share == 4:
        for c in cases:
            rows += [c] * 4
    else:
        for a, b in zip(cases[::2], cases[1::2]):
            rows += [a, b, a, b]
    f = np.array([r[0] for r in rows], np.uint32).reshape(-1)
    g = np.array([r[1] for r in rows], np.uint32).reshape(-1)
    return rows, np.stack([f, g], axis=1)


def _check_row_products(out, rows, sq, what):
    got = out.reshape(-1, 16).tolist()
    assert len(got) == len(rows)
    for j, (f, g) in enumerate(rows):
        w = row_val(f) * row_val(f if sq else g) % P
        assert row_val(got[j]) % P == w, (what, j)
        assert max(got[j]) <= ROW_CARRIED, (what, j, max(got[j]))


def check_rf_product(run, op, share=1, sq=False, trials=200):
    rows, recs = _row_records(row_cases(np.random.default_rng(20 + share + 10 * sq), trials), share)
    out = run(op, recs[:, :1] if sq else recs)
    _check_row_products(out[:, 0], rows, sq, op)


def check_rf_sqn(run):
    rows, recs = _row_records(row_cases(np.random.default_rng(31), 50))
    got = run("rf_sqn3", recs[:, :1])[:, 0].reshape(-1, 16).tolist()
    for j, (f, _) in enumerate(rows):
        assert row_val(got[j]) % P == pow(row_val(f), 8, P), j
        assert max(got[j]) <= ROW_CARRIED, j


def check_rf_lin(run):
    """rf_carry32 (limbs below 2^26), rf_sub / rf_neg (subtrahend carried),
    rf_canon on p, 2p, 2^256 - 1, on products h and on h - h"""
    rng = np.random.default_rng(32)
    cmax = [ROW_CARRIED] * 16
    big = [2**26 - 1] * 16
    cases = [(row_limbs(P), cmax), (row_limbs(2 * P), [0] * 16), (row_limbs(2**256 - 1), cmax), (big, cmax),
             ([0] * 16, [0] * 16), (row_limbs(1), row_limbs(1)), (cmax, cmax), (row_limbs(P - 1), row_limbs(P + 1)),
             (row_limbs(P + 1), row_limbs(0))]
    for i in range(16):
        cases.append(([2**26 - 1 if j == i else 0 for j in range(16)], cmax))
    while len(cases) % 16 or len(cases) < 128:
        cases.append(([int(x) for x in rng.integers(0, 2**26, 16)], [int(x) for x in rng.integers(0, ROW_CARRIED + 1, 16)]))
    rows, recs = _row_records(cases)
    out = run("rf_lin", recs)
    col = [out[:, i].reshape(-1, 16).tolist() for i in range(7)]
    for j, (f, g) in enumerate(rows):
        a, b = row_val(f), row_val(g)
        assert row_val(col[0][j]) % P == a % P and max(col[0][j]) <= ROW_CARRIED, ("carry32", j)
        assert row_val(col[1][j]) % P == (a - b) % P, ("sub", j)
        assert row_val(col[2][j]) % P == -b % P, ("neg", j)
        h = a * b % P
        assert row_val(col[6][j]) % P == h, ("mul", j)
        for k in range(16):  # the verdict is uniform within the row
            assert col[3][j][k] == (a % P == 0) + 2 * (a % P & 1), ("canon", j, k)
            assert col[4][j][k] == (h == 0) + 2 * (h & 1), ("canon(h)", j, k)
            assert col[5][j][k] == 1, ("canon(h - h)", j, k)


def check_row_moves(run):
    """ror<r>, bcast<r>, rows, the product's ror_rows triples and sum_rows on
    lane-tagged payloads; the reference is the permutation row.h defines
    (tests/host/rowcheck.cpp HostRow)."""
    rng = np.random.default_rng(33)
    nw = 16  # 4 blocks of 4 waves
    x = rng.integers(0, 2**32, (nw, 64), dtype=np.uint32)
    x = (x & 0xFFFFF000) | (np.arange(nw, dtype=np.uint32)[:, None] << 6) | np.arange(64, dtype=np.uint32)[None, :]
    lo = rng.integers(2**32 - 2**20, 2**32, (nw, 64), dtype=np.uint32)  # low words that carry
    hi = rng.integers(0, 2**32, (nw, 64), dtype=np.uint32)
    out = run("row_moves", np.stack([x.reshape(-1), lo.reshape(-1), hi.reshape(-1)], axis=1)).reshape(nw, 64, 43)
    i = np.arange(64)
    base, k = i & ~15, i & 15
    for r in range(16):
        assert np.array_equal(out[:, :, r], x[:, base | ((k - r) & 15)]), ("ror", r)
        assert np.array_equal(out[:, :, 16 + r], x[:, base | r]), ("bcast", r)
    for c in range(4):
        assert np.array_equal(out[:, :, 32 + c], x[:, 16 * c + k]), ("rows", c)
    for n, tri in enumerate(((4, 8, 12), (0, 8, 8), (12, 8, 4))):
        amt = np.array((0,) + tri)[i >> 4]
        assert np.array_equal(out[:, :, 36 + n], x[:, base | ((k - amt) & 15)]), ("ror_rows", tri)
    w = lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))
    s2 = w + w[:, i ^ 32]
    s4 = w[:, k] + w[:, 16 + k] + w[:, 32 + k] + w[:, 48 + k]
    got2 = out[:, :, 39].astype(np.uint64) | (out[:, :, 40].astype(np.uint64) << np.uint64(32))
    got4 = out[:, :, 41].astype(np.uint64) | (out[:, :, 42].astype(np.uint64) << np.uint64(32))
    assert np.array_equal(got2, s2) and np.array_equal(got4, s4)


# ---- points -----------------------------------------------------------------------------

def torsion_points():
    y = 2
    while True:
        pt = E.decode_point(y.to_bytes(32, "little"))
        y += 1
        if pt is None:
            continue
        t = E.scalar_mult(L, pt)
        if not E.is_identity(E.scalar_mult(4, t)):
            return [E.scalar_mult(k, t) for k in range(8)]


def _scaled(pt, z):
    return tuple(c * z % P for c in pt)


_POINTS = None


def point_cases():
    """64 (P, Q) pairs: B, the identity, the eight torsion points (Z = 1 and
    Z != 1), random multiples of B with Z != 1; computed once and shared"""
    global _POINTS
    if _POINTS is None:
        rng = np.random.default_rng(40)

        def rnd():
            return int.from_bytes(rng.bytes(32), "little") % P or 1

        tor = torsion_points()
        pts = [E.B, E.IDENTITY] + tor + [_scaled(t, rnd()) for t in tor] + [_scaled(E.IDENTITY, rnd())]
        while len(pts) < 64:
            pts.append(_scaled(E.scalar_mult(int.from_bytes(rng.bytes(32), "little") % L, E.B), rnd()))
        qs = [pts[int(i)] for i in rng.permutation(64)]
        qs[0], qs[1], qs[2] = E.B, E.IDENTITY, E.point_neg(pts[2])  # B + B, O + O, P + (-P)
        _POINTS = list(zip(pts, qs))
    return _POINTS


def cached(pt):
    X, Y, Z, T = pt
    return ((Y - X) % P, (Y + X) % P, 2 * Z % P, 2 * E.D * T % P)


def assert_point(got, want, what):
    X, Y, Z, T = got
    assert Z % P != 0 and E.point_equal(got, want) and (T * Z - X * Y) % P == 0, what


def check_rp(run):
    """rp_dbl, rp_add, rp_to_cached, rp_cached_neg: one point per wave, row c
    holds coordinate c"""
    pairs = point_cases()
    f = np.array([[row_limbs(c) for c in p] for p, _ in pairs], np.uint32).reshape(-1)
    g = np.array([[row_limbs(c) for c in cached(q)] for _, q in pairs], np.uint32).reshape(-1)
    out = run("rp", np.stack([f, g], axis=1))
    col = [out[:, i].reshape(len(pairs), 4, 16).tolist() for i in range(4)]
    for j, (p, q) in enumerate(pairs):
        vals = [[row_val(r) % P for r in col[i][j]] for i in range(4)]
        assert all(max(r) <= ROW_CARRIED for i in (0, 1) for r in col[i][j]), j
        assert_point(vals[0], E.point_double(p), ("rp_dbl", j))
        assert_point(vals[1], E.point_add(p, q), ("rp_add", j))
        assert tuple(vals[2]) == cached(p), ("rp_to_cached", j)
        c = cached(q)
        assert tuple(vals[3]) == (c[1], c[0], c[2], -c[3] % P), ("rp_cached_neg", j)


def check_rf_decode(run):
    """the row decode (rf_decode<0, 2>: A on rows 0, 2, R on rows 1, 3) against
    ed25519_ref's x recovery: encodings of the point cases, non-canonical y,
    y = 0, 1, p - 1, and random y (about half of them no point)"""
    rng = np.random.default_rng(41)
    ys = [(int.from_bytes(E.encode_point(p), "little") & (2**255 - 1), s) for p, _ in point_cases()[:24] for s in (0, 1)]
    ys += [(v, s) for v in (0, 1, P - 1, P, P + 1, 2**255 - 1, 2**255 - 19 + 3) for s in (0, 1)]
    while len(ys) % 32:
        ys.append((int.from_bytes(rng.bytes(32), "little") >> 1, int(rng.integers(0, 2))))
    rows = []
    for a, b in zip(ys[::2], ys[1::2]):
        rows += [a, b, a, b]
    y = np.array([row_limbs(v) for v, _ in rows], np.uint32).reshape(-1)
    s = np.repeat(np.array([sg for _, sg in rows], np.uint32), 16)
    out = run("rf_decode", np.stack([y, s], axis=1))
    xo, to, ok = (out[:, i].reshape(-1, 16).tolist() for i in range(3))
    seen = set()
    for j, (v, sg) in enumerate(rows):
        x = E._recover_x(v % P, sg)
        seen.add(x is not None)
        assert ok[j] == [int(x is not None)] * 16, j
        if x is not None:
            assert row_val(xo[j]) % P == x and row_val(to[j]) % P == x * v % P, j
    assert seen == {True, False}


# ---- quad and oct policies (DevQuad, DevOct): lane c of a quad = coordinate c -------------

QUAD_PATTERNS = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (1, 0, 2, 3), (0, 1, 2, 0), (2, 0, 0, 0),
                 (3, 2, 0, 1), (1, 2, 2, 1), (0, 3, 3, 0), (2, 3, 1, 0)]  # devcheck.hip op_q_perm
FUSED_PATTERNS = [(1, 1, 1, 1), (0, 1, 2, 0), (2, 0, 0, 0), (0, 3, 3, 0), (1, 2, 2, 1)]  # CMTV_QP_CASES


def _tagged(rng, n, width):
    """n lanes x width words, every word tagged with its lane and word index"""
    x = rng.integers(0, 2**32, (n, width), dtype=np.uint32) & np.uint32(0xFFF00000)
    return x | (np.arange(n, dtype=np.uint32)[:, None] << 4) | np.arange(width, dtype=np.uint32)[None, :]


def _src(pat, n):
    i = np.arange(n)
    return (i & ~3) | np.array(pat)[i & 3]


def check_q_perm(run):
    rng = np.random.default_rng(50)
    n = 1024  # 4 blocks of 4 waves; all 16 quads of a wave differ
    v = _tagged(rng, n, 10)
    b = rng.integers(2**31, 2**32, (n, 10), dtype=np.uint32)  # sums wrap
    out = run("q_perm", np.concatenate([v, b], axis=1))
    np_ = len(QUAD_PATTERNS)
    for p, pat in enumerate(QUAD_PATTERNS):
        s = _src(pat, n)
        assert np.array_equal(out[:, 10 * p: 10 * p + 10], v[s]), ("perm", pat)
        assert np.array_equal(out[:, 10 * np_ + p], v[s, 0]), ("perm32", pat)
        assert np.array_equal(out[:, 11 * np_ + 10 * p: 11 * np_ + 10 * p + 10], v[s] + b), ("permc", pat)


def check_q_fused(run):
    """add_perm (32-bit addition, wrapping), xor_perm, perm_lane3 (zero on
    lanes 0-2, the permuted word on lane 3) for every CMTV_QP_CASES pattern"""
    rng = np.random.default_rng(51)
    n = 1024
    v = _tagged(rng, n, 10)
    b = rng.integers(0, 2**32, (n, 10), dtype=np.uint32)
    b[::3] |= np.uint32(0xFFF00000)  # with v's random top bits: wrap-around
    k = rng.integers(0, 2**32, (n, 1), dtype=np.uint32)
    out = run("q_fused", np.concatenate([v, b, k], axis=1))
    lane3 = (np.arange(n) & 3) == 3
    for p, pat in enumerate(FUSED_PATTERNS):
        s = _src(pat, n)
        o = out[:, 30 * p: 30 * p + 30]
        assert np.array_equal(o[:, :10], v[s] + b), ("add_perm", pat)
        assert np.array_equal(o[:, 10:20], v[s] ^ k), ("xor_perm", pat)
        assert np.array_equal(o[:, 20:], np.where(lane3[:, None], v[s], np.uint32(0))), ("perm_lane3", pat)


def check_oct_upper(run):
    """from_upper / from_upper32: the lower quad of an oct (lanes with bit 2
    clear) receives lane + 4's words; the upper quad's result is unused"""
    rng = np.random.default_rng(52)
    n = 1024
    v = _tagged(rng, n, 10)
    out = run("oct_upper", v)
    low = np.nonzero((np.arange(n) & 4) == 0)[0]
    assert np.array_equal(out[low, :10], v[low + 4]) and np.array_equal(out[low, 10], v[low + 4, 0])


def check_q_point(run, fold):
    """q_dbl / q_add (FOLD as given), q_to_cached, q_cached_cneg, q_small_order:
    every quad of a wave a different point"""
    pairs = point_cases() * 4  # 256 quads: 4 blocks of 4 waves
    recs = []
    for j, (p, q) in enumerate(pairs):
        c = cached(q)
        for lane in range(4):
            recs.append(fe_limbs(p[lane]) + fe_limbs(c[lane]) + [(j // 64) & 1])
    out = run(f"q_point{fold}", recs).reshape(len(pairs), 4, 41).tolist()
    for j, (p, q) in enumerate(pairs):
        o = out[j]
        for lane in range(4):
            assert_carried(o[lane][:10], ("q_dbl", j))
            assert_carried(o[lane][10:20], ("q_add", j))
        assert_point([fe_val(o[l][:10]) % P for l in range(4)], E.point_double(p), ("q_dbl", j))
        assert_point([fe_val(o[l][10:20]) % P for l in range(4)], E.point_add(p, q), ("q_add", j))
        assert tuple(fe_val(o[l][20:30]) % P for l in range(4)) == cached(p), ("q_to_cached", j)
        c = cached(q)
        want = (c[1], c[0], c[2], -c[3] % P) if (j // 64) & 1 else c
        assert tuple(fe_val(o[l][30:40]) % P for l in range(4)) == want, ("q_cached_cneg", j)
        so = int(E.is_identity(E.scalar_mult(8, p)))
        assert [o[l][40] for l in range(4)] == [so] * 4, ("q_small_order", j)
