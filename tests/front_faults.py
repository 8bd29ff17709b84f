"""Structurally valid batches of ntx = 2 for the calls that take leaves, signatures and CompositeKey requirements as
flat arrays, and the table of single faults their argument checks must refuse (tests/test_gpu_front_faults.py).

A family is the ordered argument list of its C call behind the handles, by the header's names, and its outputs; a
fault changes one argument.  EXPECTED holds the library's return code for every (family, fault), recorded from a
named commit: literals, not computed from the code under test.
"""
import numpy as np

import tearoff_cases as T

E_ARGS, E_TOO_LARGE = -3, -5
U32_MAX = 0xFFFFFFFF
NTX = 2

u8 = lambda *a: np.array(a, np.uint8)        # noqa: E731
u32 = lambda *a: np.array(a, np.uint32)      # noqa: E731
i32 = lambda *a: np.array(a, np.int32)       # noqa: E731
u64 = lambda *a: np.array(a, np.uint64)      # noqa: E731


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _leaves():
    """Three leaves, two and one; they reach bytes [5, 40) of the arena and stand out of order."""
    return [("leaf_arena", _bytes(64, 1)), ("leaf_arena_bytes", 40), ("leaf_off", u64(5, 20, 12)),
            ("leaf_len", u32(7, 20, 8)), ("tx_leaf_begin", u32(0, 2, 3))]


def _sigs():
    return [("pk", _bytes(64, 2)), ("sig", _bytes(128, 3)), ("tx_sig_begin", u32(0, 1, 2)), ("sig_pre", None)]


def _reqs():
    """Two requirements, one each: a leaf; a node of threshold 2 over two leaves."""
    return [("nreq", 2), ("nnodes", 4), ("nchild", 2), ("kind", u8(0, 0, 0, 1)), ("leaf_key", _bytes(128, 4)),
            ("threshold", i32(0, 0, 0, 2)), ("child_begin", u32(0, 0, 0, 0, 2)), ("child", u32(1, 2)), ("weight", i32(1, 1)),
            ("req_begin", u32(0, 1, 4)), ("tx_req_begin", u32(0, 1, 2)), ("sig_key", _bytes(64, 2))]


def _tearoff(sign):
    f = T.flatten(T.service_batch(NTX, seed=31))
    args = [("ntx", NTX), ("leaf_arena", f["arena"]), ("leaf_arena_bytes", f["arena_bytes"]), ("leaf_off", f["leaf_off"]),
            ("leaf_len", f["leaf_len"]), ("tx_leaf_begin", f["txb"]), ("nnodes", len(f["kind"]))]
    args += [(k, f[k]) for k in ("kind", "left", "right", "node_hash", "tree_begin", "root")]
    if sign:
        return args + [("leaf_pre", f["leaf_pre"])], [("outcome", NTX, 1), ("first_bad", 4 * NTX, 4), ("sig_out", 64 * NTX, 1)]
    return args, [("verdict", NTX, 1), ("status", NTX, 1)]


def _notarise(validating):
    args = [("validating", int(validating)), ("ntx", NTX)] + _leaves()
    args += [("tx_input_count", u32(1, 0)), ("claimed_id", _bytes(64, 5)), ("caller", u32(0, 1)), ("tx_pre", None)]
    args += _sigs() + _reqs() + [("req_allowed", u8(0, 0))]
    ns = 1
    return args, [("outcome", NTX, 1), ("ids", 32 * NTX, 1), ("notary_sig", 64 * NTX, 1), ("first_bad", 4 * NTX, 4),
                  ("req_missing", 2, 1), ("state_conflict", ns, 1), ("consumed_id", 32 * ns, 1),
                  ("consumed_index", 4 * ns, 4), ("consumed_caller", 4 * ns, 4)]


def _resolve():
    args = [("ntx", NTX)] + _leaves() + [("claimed_id", _bytes(64, 5))] + _sigs() + _reqs()
    args += [("ninputs", 1), ("tx_input_begin", u32(0, 0, 1)), ("input_txhash", _bytes(32, 6)), ("input_index", u32(0)),
             ("tx_output_count", u32(1, 1)), ("seed", 5)]
    return args, [("outcome", NTX, 1), ("first_bad", 4 * NTX, 4), ("req_missing", 2, 1), ("bad_input", 4 * NTX, 4),
                  ("input_dep", 4, 4), ("input_status", 1, 1), ("order", 4 * NTX, 4), ("graph", 36, 4), ("ids", 32 * NTX, 1)]


def _missing_signers():
    r = dict(_reqs())
    args = [("ntx", NTX)] + [(k, r[k]) for k in ("nreq", "nnodes", "nchild")] + [("nsig", 2)]
    args += [(k, r[k]) for k in ("kind", "leaf_key", "threshold", "child_begin", "child", "weight", "req_begin",
                                 "tx_req_begin", "sig_key")]
    args += [("tx_sig_begin", u32(0, 1, 2)), ("req_allowed", u8(0, 0)), ("verdict_bitmap", None), ("wide_min", 0)]
    return args, [("req_missing", 2, 1), ("tx_status", NTX, 1)]


# family -> (the library's function, handles in front of the arguments, (arguments, outputs))
FAMILIES = {
    "notarise_validating": ("cv_notarise_batch", ("ctx", "uniq", "signer"), lambda: _notarise(True)),
    "notarise_simple": ("cv_notarise_batch", ("ctx", "uniq", "signer"), lambda: _notarise(False)),
    "filtered_verify": ("cv_filtered_verify", ("ctx",), lambda: _tearoff(False)),
    "tearoff_sign": ("cv_tearoff_sign_batch", ("ctx", "signer"), lambda: _tearoff(True)),
    "resolve": ("cv_resolve_batch", ("ctx",), _resolve),
    "missing_signers": ("cv_missing_signers", ("ctx",), _missing_signers),
}


# ---------------------------------------------------------------- the faults
def _set(name, index, value):
    def apply(a):
        a[name] = a[name].copy()
        a[name][index] = value
    return apply


def _put(name, value):
    def apply(a):
        a[name] = value
    return apply


def _ranges(name, count=None):
    """A begin array of NTX or count entries: a wrong first entry, a descending pair, and (where the count is an
    argument of its own) a last entry that is not the count."""
    out = {f"{name}[0] != 0": _set(name, 0, 1), f"{name} descends": _set(name, 1, 1000)}
    if count is not None:
        out[f"{name}'s last entry is not {count}"] = lambda a: _set(name, -1, a[count] - 1)(a)
    return out


def _no_nodes_but_children(a):
    a.update(nreq=0, nnodes=0, nchild=1, tx_req_begin=u32(0, 0, 0), req_begin=u32(0), child_begin=u32(0))


LEAF_FAULTS = {
    **_ranges("tx_leaf_begin"),
    "tx_leaf_begin null": _put("tx_leaf_begin", None),
    "nleaves 0xffffffff": _set("tx_leaf_begin", -1, U32_MAX),
    "leaf_off null": _put("leaf_off", None),
    "leaf_len null": _put("leaf_len", None),
    "leaf_arena null": _put("leaf_arena", None),
    "a leaf one byte past the arena": lambda a: a.update(leaf_arena_bytes=a["leaf_arena_bytes"] - 1),
    "a leaf whose off + len wraps": _set("leaf_off", 0, 2**64 - 3),
}
SIG_FAULTS = {
    **_ranges("tx_sig_begin"),
    "tx_sig_begin null": _put("tx_sig_begin", None),
    "nsig 0xffffffff": _set("tx_sig_begin", -1, U32_MAX),
    "pk null": _put("pk", None),
    "sig null": _put("sig", None),
    "sig_key null": _put("sig_key", None),
}
KEY_FAULTS = {                        # cv_missing_signers: the signers' keys alone, nsig an argument
    **_ranges("tx_sig_begin", "nsig"),
    "tx_sig_begin null": _put("tx_sig_begin", None),
    "nsig 0xffffffff": _put("nsig", U32_MAX),
    "sig_key null": _put("sig_key", None),
}
REQ_FAULTS = {
    **_ranges("tx_req_begin", "nreq"), **_ranges("req_begin", "nnodes"),
    **{f"{k} null": _put(k, None) for k in ("kind", "leaf_key", "threshold", "child_begin", "child", "weight",
                                            "req_begin", "tx_req_begin")},
    **{f"{k} 0xffffffff": _put(k, U32_MAX) for k in ("nreq", "nnodes", "nchild")},
    "child_begin[0] != 0": _set("child_begin", 0, 1),
    "child_begin's last entry is not nchild": _set("child_begin", -1, 1),
    "no nodes but children": _no_nodes_but_children,
}
FAULTS = {
    "notarise_validating": {**LEAF_FAULTS, **SIG_FAULTS, **REQ_FAULTS},
    "notarise_simple": LEAF_FAULTS,
    "filtered_verify": LEAF_FAULTS,
    "tearoff_sign": LEAF_FAULTS,
    "resolve": {**LEAF_FAULTS, **SIG_FAULTS, **REQ_FAULTS},
    "missing_signers": {**KEY_FAULTS, **REQ_FAULTS},
}

# Recorded by running this table with NULL handles (every check comes before the context's) against the library built
# from commit a827704: the five faults below gave CV_E_TOO_LARGE in
# every family that has them, all the others CV_E_ARGS.
TOO_LARGE = {"nleaves 0xffffffff", "nsig 0xffffffff", "nreq 0xffffffff", "nnodes 0xffffffff", "nchild 0xffffffff"}
# every other fault of every family: CV_E_ARGS
EXPECTED = {(fam, fault): E_TOO_LARGE if fault in TOO_LARGE else E_ARGS for fam, faults in FAULTS.items() for fault in faults}


def call(lib, P, family, handles, args, outs):
    """The family's C call: args by name in the call's order, arrays by address, None as NULL; outs: addresses."""
    fn, names, _ = FAMILIES[family]
    vals = [P(v) if isinstance(v, np.ndarray) else v for v in args.values()]
    return getattr(lib, fn)(*[handles[h] for h in names], *vals, *outs)
