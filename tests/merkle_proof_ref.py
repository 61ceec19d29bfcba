"""Reference for the merkle proof tests, restated from crypto/merkle/proof.go
in its own recursive form (the device code uses the level form and an
iterative walk, so the two sides stay structurally independent). Nothing
here goes through the library.

  ProofsFromByteSlices      proof.go:35-48, trailsFromByteSlices :232-252, FlattenAunts :213-228
  Proof.Verify              proof.go:52-74
  computeHashFromAunts      proof.go:166-197
  Proof.ValidateBasic       proof.go:113-132
  Txs.Proof, TxProof        types/tx.go:80-124
  NewPartSetFromData        types/part_set.go:166-190
"""
from merkle_ref import EMPTY_ROOT, inner_hash, leaf_hash, sha256, split_point

MAX_AUNTS = 100

# cmtv_merkle_proofs_verify's statuses, in Verify's order of checks
OK, ENEGTOTAL, ENEGINDEX, ELEAF, EINDEX, EEXTRA, EMISSING, EROOT = range(8)


class Node:
    """proof.go ProofNode: one of left / right is the sibling, unless this is the root."""

    def __init__(self, h):
        self.hash, self.parent, self.left, self.right = h, None, None, None

    def flatten_aunts(self):
        out, n = [], self
        while n is not None:
            if n.left is not None:
                out.append(n.left.hash)
            elif n.right is not None:
                out.append(n.right.hash)
            n = n.parent
        return out


def trails(leaf_hashes):
    """trailsFromByteSlices over leaves already hashed: (leaf nodes, root node)."""
    n = len(leaf_hashes)
    if n == 0:
        return [], Node(EMPTY_ROOT)
    if n == 1:
        t = Node(leaf_hashes[0])
        return [t], t
    k = split_point(n)
    lefts, lroot = trails(leaf_hashes[:k])
    rights, rroot = trails(leaf_hashes[k:])
    root = Node(inner_hash(lroot.hash, rroot.hash))
    lroot.parent, lroot.right = root, rroot
    rroot.parent, rroot.left = root, lroot
    return lefts + rights, root


def proofs_from_leaf_hashes(leaf_hashes):
    """(root, [(total, index, leaf_hash, aunts)])."""
    ts, root = trails(list(leaf_hashes))
    return root.hash, [(len(ts), i, t.hash, t.flatten_aunts()) for i, t in enumerate(ts)]


def proofs_from_byte_slices(items):
    return proofs_from_leaf_hashes([leaf_hash(it) for it in items])


def txs_proofs(txs):
    """Txs.Proof(i) for every i: the items are SHA-256(tx)."""
    return proofs_from_byte_slices([sha256(tx) for tx in txs])


def parts(data, part_size):
    total = (len(data) + part_size - 1) // part_size
    return [data[i * part_size: min(len(data), (i + 1) * part_size)] for i in range(total)]


def proof_len(total, index):
    """How many aunts leaf index of a tree of total leaves has, by the recursive split."""
    k = 0
    while total > 1:
        sp = split_point(total)
        if index < sp:
            total = sp
        else:
            index, total = index - sp, total - sp
        k += 1
    return k


class ProofError(Exception):
    def __init__(self, status, msg):
        super().__init__(msg)
        self.status = status


def hash_from_aunts(index, total, leaf_h, aunts):
    """computeHashFromAunts, recursive from the top."""
    if index >= total or index < 0 or total <= 0:
        raise ProofError(EINDEX, f"invalid index {index} and/or total {total}")
    if total == 1:
        if len(aunts) != 0:
            raise ProofError(EEXTRA, "unexpected inner hashes")
        return leaf_h
    if len(aunts) == 0:
        raise ProofError(EMISSING, "expected at least one inner hash")
    k = split_point(total)
    if index < k:
        return inner_hash(hash_from_aunts(index, k, leaf_h, aunts[:-1]), aunts[-1])
    return inner_hash(aunts[-1], hash_from_aunts(index - k, total - k, leaf_h, aunts[:-1]))


def verify(total, index, leaf_h, aunts, root, leaf, tx=False):
    """Proof.Verify: (status, error string or None, out_hash as the C call
    reports it). leaf None: no leaf check; root None: no root check (both are
    the C call's options, not the reference's). tx: the leaf is SHA-256(leaf)."""
    zero = bytes(32)
    if total < 0:
        return ENEGTOTAL, "proof total must be positive", zero
    if index < 0:
        return ENEGINDEX, "proof index cannot be negative", zero
    if leaf is not None:
        lh = leaf_hash(sha256(leaf) if tx else leaf)
        if lh != leaf_h:
            return ELEAF, f"invalid leaf hash: wanted {lh.hex().upper()} got {leaf_h.hex().upper()}", lh
    try:
        computed = hash_from_aunts(index, total, leaf_h, list(aunts))
    except ProofError as e:
        return e.status, f"compute root hash: {e}", zero
    if root is not None and computed != root:
        return EROOT, f"invalid root hash: wanted {root.hex().upper()} got {computed.hex().upper()}", computed
    return OK, None, computed


def validate_basic(total, index, leaf_h, aunts):
    """Proof.ValidateBasic: the error string or None."""
    if total < 0:
        return "negative Total"
    if index < 0:
        return "negative Index"
    if len(leaf_h) != 32:
        return f"expected LeafHash size to be 32, got {len(leaf_h)}"
    if len(aunts) > MAX_AUNTS:
        return f"expected no more than {MAX_AUNTS} aunts, got {len(aunts)}"
    for i, a in enumerate(aunts):
        if len(a) != 32:
            return f"expected Aunts#{i} size to be 32, got {len(a)}"
    return None


def tx_proof_validate(root_hash, data, proof, data_hash):
    """TxProof.Validate: the error string or None. proof: (total, index, leaf_hash, aunts)."""
    if data_hash != root_hash:
        return "proof matches different data hash"
    if proof[1] < 0:
        return "proof index cannot be negative"
    if proof[0] <= 0:
        return "proof total must be positive"
    if verify(*proof, root_hash, data, tx=True)[0] != OK:
        return "proof is not internally consistent"
    return None
