"""Cases and the reference restatement for cv_filtered_verify and cv_tearoff_sign_batch, shared by
tests/test_tearoff_cpu.py (the lane functions of corda_amd/csrc/cv_tearoff.h on the CPU) and the GPU tests
(tests/test_gpu_tearoff.py, tests/test_gpu_tearoff_output_contract.py).  No GPU, nothing of corda_amd.

oracle_sign() restates NodeInterestRates.Oracle.sign(ftx, merkleRoot) (samples/irs-demo/src/main/kotlin/net/corda/irs/
api/NodeInterestRates.kt:190-225) over plain data AS THE REFERENCE'S CONTROL FLOW: it raises where the reference throws,
in its order.  Hashing and the tree verify are oracle/merkle_ref.py's (sha256, filtered_verify, verify_flat).

A filtered leaf is a dict: group ("inputs" | "outputs" | "attachments" | "commands"), blob (its serialised bytes),
vouched (a command only: it is a Fix and the oracle is among its signers), known (a vouched command only: the oracle
knows the fix as given).  A tear-off is a dict: leaves (the filtered leaves in getFilteredHashes order), nodes (kind,
left, right, hashes: its partial tree in the flat encoding, indices from 0), root (32 bytes), tree (the merkle_ref
object the nodes were flattened from, or None when the nodes were tampered with).
"""
import numpy as np

import merkle_ref as M

SUCCESS, NO_LEAVES, MALFORMED, VERIFY_FAILED, NOT_COMMANDS, WRONG_COMMAND, UNKNOWN = range(7)
NO_LEAF = 0xFFFFFFFF
PMT_OK, PMT_MALFORMED, PMT_NO_INCLUDED = 0, 2, 4
GROUPS = ("inputs", "outputs", "attachments", "commands")
BLOB_LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 300)      # around SHA-256's padding seams, and several blocks


class IllegalArgumentException(Exception):
    def __init__(self, outcome, leaf=None):
        super().__init__(outcome, leaf)
        self.outcome, self.leaf = outcome, leaf


class UnknownFix(Exception):
    def __init__(self, leaf):
        super().__init__(leaf)
        self.leaf = leaf


def leaf(blob, group="commands", vouched=True, known=True):
    return {"blob": bytes(blob), "group": group, "vouched": vouched, "known": known}


def classify(lf):
    """leaf_pre: what the binding passes for the leaf (include/cordaverify.h)."""
    if lf["group"] != "commands":
        return 1
    if not lf["vouched"]:
        return 2
    return 0 if lf["known"] else 3


# ---------------------------------------------------------------- the restatement
def filtered_verify(tx):
    """FilteredTransaction.verify(merkleRoot) (MerkleTransaction.kt:173-178) -> bool; raises MerkleTreeException for no
    leaves and IllegalArgumentException(MALFORMED) where the nodes are no tree (the shim's rule: no PartialTree object
    can be built from them)."""
    hashes = [M.sha256(lf["blob"]) for lf in tx["leaves"]]          # FilteredLeaves.getFilteredHashes, :112-117
    k, l, r, h = tx["nodes"]
    if tx["tree"] is not None:
        ok = M.filtered_verify(tx["tree"], tx["root"], hashes)
        assert M.verify_flat(k, l, r, h, 0, len(k), tx["root"], hashes) == (int(ok), 0)
        return ok
    if len(hashes) == 0:
        raise M.MerkleTreeException("Transaction without included leaves.")
    v, st = M.verify_flat(k, l, r, h, 0, len(k), tx["root"], hashes)
    if st:
        raise IllegalArgumentException(MALFORMED)
    return bool(v)


def oracle_sign(tx):
    """Oracle.sign: returns True where the reference signs merkleRoot.bytes, raises what it throws otherwise."""
    if not filtered_verify(tx):                                                           # :191
        raise M.MerkleTreeException("Rate Fix Oracle: Couldn't verify partial Merkle tree.")
    leaves = tx["leaves"]
    # :195-197 require(leaves.inputs.isEmpty() && leaves.outputs.isEmpty() && leaves.attachments.isEmpty())
    for i, lf in enumerate(leaves):
        if lf["group"] != "commands":
            raise IllegalArgumentException(NOT_COMMANDS, i)
    commands = list(enumerate(leaves))
    fixes = [(i, c) for i, c in commands if c["vouched"]]                                 # :199-201
    if len(fixes) != len(commands):                                                       # :204-205
        raise IllegalArgumentException(WRONG_COMMAND, next(i for i, c in commands if not c["vouched"]))
    if not fixes:                                                                         # :208-209
        raise AssertionError("unreachable: there is a leaf and every leaf is a vouched-for command")
    for i, fix in fixes:                                                                  # :213-217
        if not fix["known"]:
            raise UnknownFix(i)
    return True                                                                           # :224


def expected(txs):
    """-> dict: outcome u8[ntx], first_bad u32[ntx] (absolute leaf indices), accepted u32[], verdict and status of
    cv_filtered_verify — one sequential Oracle.sign after another."""
    n = len(txs)
    out, fb = np.zeros(n, np.uint8), np.full(n, NO_LEAF, np.uint32)
    verdict, status = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    base = 0
    for t, tx in enumerate(txs):
        try:
            verdict[t] = filtered_verify(tx)
        except M.MerkleTreeException:
            status[t] = PMT_NO_INCLUDED
        except IllegalArgumentException:
            status[t] = PMT_MALFORMED
        try:
            oracle_sign(tx)
        except M.MerkleTreeException as e:
            out[t] = NO_LEAVES if e.reason == "Transaction without included leaves." else VERIFY_FAILED
        except IllegalArgumentException as e:
            out[t] = e.outcome
            if e.leaf is not None:
                fb[t] = base + e.leaf
        except UnknownFix as e:
            out[t], fb[t] = UNKNOWN, base + e.leaf
        base += len(tx["leaves"])
    return {"outcome": out, "first_bad": fb, "accepted": np.nonzero(out == SUCCESS)[0].astype(np.uint32),
            "verdict": verdict, "status": status}


def python_gate(txb, verdict, status, leaf_pre):
    """The gate between cv_filtered_verify and cv_ed25519_sign_keyed as a binding composes them: (outcome, first_bad)
    from the verify's results and leaf_pre (or None)."""
    n = len(txb) - 1
    out, fb = np.zeros(n, np.uint8), np.full(n, NO_LEAF, np.uint32)
    for t in range(n):
        b, e = int(txb[t]), int(txb[t + 1])
        if status[t] == PMT_NO_INCLUDED:
            out[t] = NO_LEAVES
        elif status[t] != PMT_OK:
            out[t] = MALFORMED
        elif not verdict[t]:
            out[t] = VERIFY_FAILED
        elif leaf_pre is not None:
            for cls in (1, 2, 3):
                hit = np.nonzero(leaf_pre[b:e] == cls)[0]
                if hit.size:
                    out[t], fb[t] = VERIFY_FAILED + cls, b + int(hit[0])
                    break
    return out, fb


# ---------------------------------------------------------------- building tear-offs
def tearoff(all_leaves, keep, root=None):
    """The tear-off of a transaction whose leaves are all_leaves (in group order), keeping the leaves at `keep`."""
    hashes = [M.sha256(lf["blob"]) for lf in all_leaves]
    full = M.get_merkle_tree(hashes)
    tree = M.build_partial(full, [hashes[i] for i in keep])
    return {"leaves": [all_leaves[i] for i in keep], "nodes": M.flatten(tree), "root": full.hash if root is None else root,
            "tree": tree}


def tampered(tx, **kw):
    """A copy with leaves, nodes or root replaced (nodes replaced: no tree object stands behind them any more)."""
    out = dict(tx, **kw)
    if "nodes" in kw:
        out["tree"] = None
    return out


def flip(b, at=0):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def blobs(n, seed, lengths=BLOB_LENGTHS):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, lengths[(seed + i) % len(lengths)], dtype=np.uint8)) for i in range(n)]


def wire(nleaves, seed, ncommands=None):
    """The leaves of a transaction: nleaves distinct blobs of the listed lengths, the last ncommands of them commands
    (default: all), the others inputs."""
    bs = blobs(nleaves, seed)
    bs = [b + bytes([i]) if bs.count(b) > 1 else b for i, b in enumerate(bs)]      # distinct (two empty blobs)
    nc = nleaves if ncommands is None else ncommands
    return [leaf(b, "inputs" if i < nleaves - nc else "commands") for i, b in enumerate(bs)]


def flatten(txs):
    """-> dict: the arrays of Engine.filtered_verify / Engine.tearoff_sign_batch."""
    arena, off, ln, txb, pre = bytearray(), [], [], [0], []
    kind, left, right, hashes, tb, roots = [], [], [], [], [0], []
    for tx in txs:
        for lf in tx["leaves"]:
            off.append(len(arena))
            ln.append(len(lf["blob"]))
            arena += lf["blob"]
            pre.append(classify(lf))
        txb.append(len(off))
        k, l, r, h = tx["nodes"]
        base = len(kind)
        kind += k
        left += [x + base if kk == M.NODE else x for x, kk in zip(l, k)]
        right += [x + base if kk == M.NODE else x for x, kk in zip(r, k)]
        hashes += h
        tb.append(len(kind))
        roots.append(tx["root"])
    rows = lambda bs: np.frombuffer(b"".join(bs), np.uint8).reshape(-1, 32).copy()      # noqa: E731
    return {"ntx": len(txs), "arena": np.frombuffer(bytes(arena) + bytes(16), np.uint8).copy(), "arena_bytes": len(arena),
            "leaf_off": np.array(off, np.uint64), "leaf_len": np.array(ln, np.uint32), "txb": np.array(txb, np.uint32),
            "kind": np.array(kind, np.uint8), "left": np.array(left, np.uint32), "right": np.array(right, np.uint32),
            "node_hash": rows(hashes) if hashes else np.zeros((0, 32), np.uint8), "tree_begin": np.array(tb, np.uint32),
            "root": rows(roots), "leaf_pre": np.array(pre, np.uint8)}


# ---------------------------------------------------------------- the cases
def precedence_cases():
    """Every combination of: no leaves, malformed nodes, a wrong root, and the presence of a leaf of class 1, 2 and 3,
    where the combination is possible (without leaves there is no class): 4 + 32 combinations; where classes 2 and 3
    meet, both orders of their leaves.  The classes come twice each, so `first` means something."""
    txs = []
    for empty in (0, 1):
        for malformed in (0, 1):
            for wrong_root in (0, 1):
                for mask in range(1 if empty else 8):
                    for swap in ((0, 1) if mask & 6 == 6 else (0,)):
                        seed = len(txs)
                        w = wire(9, seed, ncommands=6)
                        # leaves 0-2 inputs, 3-8 commands; kept: a fine command always, then what the mask asks for
                        keep = [] if empty else [3]
                        if mask & 1:
                            keep += [0, 2]
                        two, three = ([4, 7], [5, 8]) if not swap else ([5, 8], [4, 7])
                        if mask & 2:
                            keep += two
                            for i in two:
                                w[i] = dict(w[i], vouched=False, known=bool(i & 1))
                        if mask & 4:
                            keep += three
                            for i in three:
                                w[i] = dict(w[i], known=False)
                        tx = tearoff(w, sorted(keep))
                        if wrong_root:
                            tx = tampered(tx, root=flip(tx["root"], seed % 32))
                        if malformed:
                            k, l, r, h = tx["nodes"]
                            tx = tampered(tx, nodes=([7] + list(k[1:]), l, r, h))
                        txs.append(tx)
    return txs


def one_leaf(seed, **kw):
    """A tear-off of a one-leaf transaction: one IncludedLeaf, the root its hash."""
    return tearoff([leaf(blobs(1, seed)[0] + seed.to_bytes(4, "little"), **kw)], [0])


def refused(kind, seed):
    """A one-node tear-off with outcome `kind` (1-6)."""
    if kind == NO_LEAVES:
        return tearoff([leaf(b"only" + seed.to_bytes(4, "little"))], [])
    if kind == MALFORMED:
        tx = one_leaf(seed)
        k, l, r, h = tx["nodes"]
        return tampered(tx, nodes=([9], l, r, h))
    if kind == VERIFY_FAILED:
        tx = one_leaf(seed)
        return tampered(tx, root=flip(tx["root"], seed % 32))
    if kind == NOT_COMMANDS:
        return one_leaf(seed, group=GROUPS[seed % 3])
    if kind == WRONG_COMMAND:
        return one_leaf(seed, vouched=False)
    return one_leaf(seed, known=False)


def edge_batches():
    """Small batches at which pieces of the calls' one buffer are empty or nothing is signed: one tear-off with no
    leaf and no node at all (L = M = 0), the same beside two ordinary ones, and three tear-offs all refused."""
    bare = {"leaves": [], "nodes": ([], [], [], []), "root": bytes(range(32)), "tree": None}
    return {"bare": [bare], "bare_between": [one_leaf(21), bare, refused(UNKNOWN, 22)],
            "three_refused": [refused(NO_LEAVES, 31), refused(VERIFY_FAILED, 32), refused(WRONG_COMMAND, 33)]}


def service_batch(ntx, seed=0):
    """ntx tear-offs, roughly 1 in 8 refused, cycling through outcomes 1 to 6; up to 64 the accepted ones are
    tear-offs of 6-leaf transactions with 2 kept commands, above that one-node trees."""
    txs = []
    for t in range(ntx):
        if t % 8 == 3:
            txs.append(refused(1 + (t // 8) % 6, seed + t))
        elif ntx <= 64:
            txs.append(tearoff(wire(6, seed + t, ncommands=3), [3, 5]))
        else:
            txs.append(one_leaf(seed + t))
    return txs
