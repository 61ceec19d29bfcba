"""cometbft_amd -- MI355X-native (gfx950) batch Ed25519 (and sr25519, and
secp256k1 ECDSA) verifier for CometBFT's commit-verification hot path.

The product is libcmtverify.so (C ABI in include/cmtverify.h): HIP kernels that
verify one signature per lane, a host runtime (streams, pinned staging) and a
C++ replay of ValidatorSet.VerifyCommit* over device verdicts. This package is
the Python binding used by tests and bench.py; see DESIGN.md.
"""
from . import _native
from .crypto import (MODE_GO_STDLIB, MODE_ZIP215, BatchVerifier, Context, KeySet, PubKey, Secp256k1BatchVerifier,
                     Secp256k1KeySet, Secp256k1PubKey, Sr25519BatchVerifier, Sr25519PubKey, default_context, new_batch_verifier,
                     pack_messages)
from .types import (Header, Proof, TxProof, commit_hashes, header_hashes, merkle_root, merkle_roots, part_set_from_data,
                    proofs_from_byte_slices, proofs_from_trees, txs_hash, txs_hashes, txs_proofs, valset_hashes,
                    verify_proofs)

__all__ = ["Header", "commit_hashes", "header_hashes", "merkle_root", "merkle_roots", "txs_hash", "txs_hashes",
           "valset_hashes", "Proof", "TxProof", "part_set_from_data", "proofs_from_byte_slices", "proofs_from_trees",
           "txs_proofs", "verify_proofs", "MODE_GO_STDLIB", "MODE_ZIP215", "BatchVerifier", "Context", "KeySet", "PubKey", "Secp256k1BatchVerifier",
           "Secp256k1KeySet", "Secp256k1PubKey", "Sr25519BatchVerifier", "Sr25519PubKey", "default_context", "new_batch_verifier",
           "pack_messages", "_native"]
