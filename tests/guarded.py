"""Poisoned, guard-banded output buffers for the output-contract tests (tests/test_gpu_output_contract.py on the
device-resident API, tests/test_gpu_host_output_contract.py on the host-buffer C-ABI).

`Guarded` carves named outputs out of ONE larger allocation, a torch.uint8 device tensor or a numpy array (pageable,
or pinned when the caller hands in Engine.host_empty as `alloc`).  Every output
  - starts at an address that has the alignment the caller asks for and NOT twice that alignment (a bitmap of
    alignment 8 lies at 8 mod 16, a status array of alignment 1 at an odd address), so code that quietly assumes
    more than the contract states is exercised at the contract's minimum — never below it;
  - has at least GUARD bytes of guard before it and after it;
  - is filled, like the guards, with the caller's byte, so a result that is ORed in, or left alone where the
    header promises a value, shows.
check_guards() names the first guard byte that changed by output and offset.

The alignments of the device-resident API (include/cordaverify.h states them; the kernels' vector accesses need
them) are collected in DEVICE_ALIGN.
"""
import numpy as np

GUARD = 256
CV_SIG_BAD_KEY = 1

# per-pointer alignment of the device-resident API, as include/cordaverify.h states it
DEVICE_ALIGN = {
    "d_pk": 16, "d_sig": 16, "d_keys": 16, "d_seed": 16,      # 16-byte vector loads and stores of the records
    "d_ids": 16, "d_workspace": 16,                          # 16-byte stores of ids and leaf digests
    "d_bitmap": 8,                                           # whole 64-bit words, 64-bit atomics
    "d_off": 8, "d_leaf_off": 8,                             # uint64
    "d_len": 4, "d_leaf_len": 4, "d_key_index": 4, "d_tx_leaf_begin": 4,   # uint32
    "d_status": 1, "d_tx_status": 1, "d_arena": 1,           # bytes
}


class GuardError(AssertionError):
    pass


class Guarded:
    """outputs: a list of (name, nbytes, align); fill: the poison byte; device: a torch device string for a device
    tensor, None for host memory; alloc: for host memory, a function nbytes -> uint8 numpy array (default np.empty)."""

    def __init__(self, outputs, fill, device=None, alloc=None):
        self.fill = int(fill) & 0xFF
        self.device = device
        for name, nbytes, align in outputs:
            if align < 1 or align & (align - 1) or nbytes < 0:
                raise ValueError(f"{name}: bad size or alignment")
        total = GUARD + sum(GUARD + 3 * a + nb for _, nb, a in outputs)       # up to 3 * align - 1 bytes of padding each
        if device is not None:
            import torch
            self._torch = torch
            self.buf = torch.full((total,), self.fill, dtype=torch.uint8, device=device)
            self.base = self.buf.data_ptr()
        else:
            self.buf = np.empty(total, np.uint8) if alloc is None else alloc(total).reshape(-1).view(np.uint8)
            self.buf[:] = self.fill
            self.base = self.buf.ctypes.data
        self.total = total
        self.slots = {}            # name -> (offset, nbytes, align)
        self.order = []
        cur = self.base            # the first address not yet given out
        for name, nbytes, align in outputs:
            a = cur + GUARD
            a = (a + 2 * align - 1) // (2 * align) * (2 * align) + align     # a = align (mod 2 * align)
            assert a % align == 0 and a % (2 * align) == align and a - cur >= GUARD
            self.slots[name] = (a - self.base, nbytes, align)
            self.order.append(name)
            cur = a + nbytes
        assert cur + GUARD <= self.base + total

    # ------------------------------------------------------------ the outputs
    def ptr(self, name) -> int:
        """The output's address (what the C-ABI gets)."""
        return self.base + self.slots[name][0]

    def snapshot(self):
        """Device tensor: copy the allocation to the host once; read() and the guard check then use that copy
        (until refill()) instead of one copy each.  The caller has synchronised with the work that writes it."""
        if self.device is not None:
            self._snap = self.buf.cpu().numpy()
        return self

    def _host(self) -> np.ndarray:
        if self.device is None:
            return self.buf
        snap = getattr(self, "_snap", None)
        return snap if snap is not None else self.buf.cpu().numpy()

    def read(self, name, dtype=np.uint8, shape=None) -> np.ndarray:
        """A host COPY of the output's bytes as dtype (the copy is aligned whatever the output's address is)."""
        off, nbytes, _ = self.slots[name]
        a = np.array(self._host()[off:off + nbytes], copy=True).view(dtype)
        return a if shape is None else a.reshape(shape)

    def untouched(self, name) -> bool:
        """Every byte of the output still holds the fill."""
        return bool((self.read(name) == self.fill).all())

    def refill(self):
        """Poison guards and outputs again (between two calls on one allocation)."""
        if self.device is not None:
            self._snap = None
            self.buf.fill_(self.fill)
        else:
            self.buf[:] = self.fill

    # ------------------------------------------------------------ the guards
    def first_changed_guard(self):
        """None, or (name, where, offset, value): the first changed guard byte in address order — where = "after":
        offset bytes past the output's end (0 = the byte right behind it), "before": offset bytes before its
        start (1 = the byte right in front of it)."""
        h = self._host()
        mask = np.ones(self.total, bool)
        for off, nbytes, _ in self.slots.values():
            mask[off:off + nbytes] = False
        bad = np.nonzero(mask & (h != self.fill))[0]
        if bad.size == 0:
            return None
        p = int(bad[0])
        prev = None
        for name in self.order:
            off, nbytes, _ = self.slots[name]
            if p < off:
                if prev is not None and p - prev[1] < GUARD:
                    return prev[0], "after", p - prev[1], int(h[p])
                return name, "before", off - p, int(h[p])
            prev = (name, off + nbytes)
        return prev[0], "after", p - prev[1], int(h[p])

    def check_guards(self, what=""):
        bad = self.first_changed_guard()
        if bad is not None:
            name, where, offset, value = bad
            raise GuardError(f"{what}: guard byte {offset} {where} output '{name}' changed from "
                             f"0x{self.fill:02x} to 0x{value:02x}")


class Options:
    """Per-context options (cv_set_option) set for the block and restored after it."""

    def __init__(self, engine, **kw):
        self.e, self.kw = engine, kw

    def __enter__(self):
        self.old = {k: self.e.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            self.e.set_option(k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.e.set_option(k, v)


def corpus_rows(corpus, n, last, seed=0):
    """n rows of the corpus in a seeded order: the last one accepted (`accepted`) or a CV_SIG_BAD_KEY row
    (`bad_key`); from two records up the first one is of the other kind, so every such batch holds an accepted
    signature and a key that is not a point.  n above the corpus: the order tiled."""
    m = len(corpus["pk"])
    perm = np.random.default_rng(7919 * n + seed).permutation(m)
    acc, bad = corpus["verdict"] == 1, corpus["status"] == CV_SIG_BAD_KEY
    want_last, want_first = (acc, bad) if last == "accepted" else (bad, acc)
    p_last = (n - 1) % m
    j = int(np.nonzero(want_last[perm])[0][0])
    perm[[j, p_last]] = perm[[p_last, j]]
    if n >= 2:
        cand = [int(k) for k in np.nonzero(want_first[perm])[0] if k != p_last]
        perm[[cand[0], 0]] = perm[[0, cand[0]]]
    rows = perm[np.arange(n) % m]
    # the conditions the cases rest on, from the fixture's own columns
    assert want_last[rows[-1]] and (n < 2 or want_first[rows[0]])
    assert not (acc & bad).any()
    return rows


def tail_bits(bitmap_words: np.ndarray, n: int) -> int:
    """The bits of the last bitmap word at and above n (0 when n is a multiple of 64 or they are all zero)."""
    return int(bitmap_words[-1]) >> (n % 64) if n % 64 else 0
