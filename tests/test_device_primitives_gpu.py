"""The device-only code paths on an MI355X, primitive by primitive, against
Python integers: tests/dev/devcheck (a stand-alone gfx950 program over the
product headers, not linked with libcmtverify.so) runs one small kernel per
op and returns raw words; tests/dev/devcases.py builds the cases -- operands
exactly at the bounds the headers state (MUL_BOUND - 1, SQ_ODD_BOUND - 1:
fe25519.h; 676999 and 0x10000 + 128: row.h, tests/host/rowcheck.cpp), whole
waves of different values per lane, row and quad -- and compares exactly.

What only the device has, and the end-to-end verdict tests reach only with
effectively random limbs: the __HIP_DEVICE_COMPILE__ branches (alignbit /
bitop3 / alignbyte in sha512.h, keccak.h's rotate, CMTV_XOR_AND, hs_clz,
hs_udiv31, the UNI ballot branches), DevRow's inline-asm products and
permlane row moves (row_dev.h), DevQuad / DevOct's DPP blocks (devtables.h).

Each test starts one child process, one at a time; a child that fails,
faults or times out fails the test and is not run again.

What the checks catch, tried once with arithmetic-only edits of the headers
(devcheck rebuilt from the edited copy, run on an MI355X; "before": the tests
this file came after):
  one wrap twist in RowCtx (tw[7]: 38 -> 19)
      fails test_row_product[rf_mul], [rf_sq], test_row_sqn,
      test_row_carry_sub_neg_canon, test_row_point_formulas (the split
      products use tw4 / tw8 and pass). Before: test_host_math's row tests
      and the GPU corpus parity failed too.
  the 19 c fold dropped from fe_reduce64
      fails test_lane_primitive[fe_mul, fe_sq, fe_sqn*, fe_add_sub_neg,
      fe_invert_pow22523], test_quad_point_formulas (and the same host
      checks). Before: 32 of test_host_math's 35 failed too.
  one CMTV_QP_CASES string ([0,3,3,0] -> [0,3,2,0])
      fails test_quad_fused_dpp_blocks, test_quad_point_formulas[2]. Before:
      none -- the library builds FOLD = 0, which never instantiates the blocks.
  funnel_bytes' alignbyte shift off by one
      fails test_lane_primitive[sha512_prefixed_16, sha512_prefixed_8]. Before:
      no CPU test (device branch); the GPU tests were not run against it.
  hs_udiv31 rounding up
      fails test_lane_primitive[hs_udiv31_clz] (and the host check) only:
      the decomposition's output does not change (Lehmer's corner check
      rejects the quotient, the exact Euclid steps give the same pair).
      Before: no CPU test failed; the GPU tests were not run against it.

The verdicts' rejection rules as primitives (test_lane_primitive[ristretto_decode,
fe_sqrt_ratio_m1, secp_parse_pubkey, secp_sig_scalars, secp_x_is_r, pt_add,
pt_double]): each rule of sr25519.h's ristretto_decode and of secp256k1.h's
key parser, scalar checks and final comparison, removed alone on a CPU host
build, fails one of them or a corpus test; was_square, r = 0 and `wraps` in
secp_x_is_r are pinned by these alone. The table is DESIGN.md section 2.1."""
import pytest

from tests.dev import devbuild, devcases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return devcases.runner(devbuild.build())


# ---- (a), (d): the lane layer, scalars and hashes (also run on the host build) ----------

@pytest.mark.parametrize("name", list(devcases.LANE_CHECKS))
def test_lane_primitive(run, name):
    devcases.LANE_CHECKS[name](run)


@pytest.mark.parametrize("odd", [True, False])
def test_half_scalars_uniform(run, odd):
    """half_scalars<true, true> (every lane of a wave the same scalar, branch
    conditions from the ballot): byte-identical to halfcheck, all lanes agree"""
    devcases.check_half(run, odd, uni=True)


# ---- (b): the row layer through DevRow -----------------------------------------------------

@pytest.mark.parametrize("op,share,sq", [("rf_mul", 1, False), ("rf_sq", 1, True), ("rf_mul_s2", 2, False),
                                         ("rf_mul_s4", 4, False), ("rf_sq_s2", 2, True), ("rf_sq_s4", 4, True)])
def test_row_product(run, op, share, sq):
    devcases.check_rf_product(run, op, share, sq)


def test_row_sqn(run):
    devcases.check_rf_sqn(run)


def test_row_carry_sub_neg_canon(run):
    devcases.check_rf_lin(run)


def test_row_moves(run):
    devcases.check_row_moves(run)


def test_row_point_formulas(run):
    devcases.check_rp(run)


def test_row_decode(run):
    devcases.check_rf_decode(run)


# ---- (c): the quad and oct policies ----------------------------------------------------------

def test_quad_perm_patterns(run):
    devcases.check_q_perm(run)


def test_quad_fused_dpp_blocks(run):
    devcases.check_q_fused(run)


def test_oct_from_upper(run):
    devcases.check_oct_upper(run)


@pytest.mark.parametrize("fold", [0, 2])
def test_quad_point_formulas(run, fold):
    """FOLD = 0 is what the library builds (CMTV_DPP_FOLD); FOLD = 2 runs the
    formulas through add_perm / xor_perm / perm_lane3"""
    devcases.check_q_point(run, fold)
