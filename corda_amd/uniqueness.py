"""Uniqueness providers of the notary commit step.

The reference commits the inputs of ONE transaction per notary flow:
  UniquenessProvider.commit(states, txId, callerIdentity)   core/.../node/services/UniquenessProvider.kt:15
  InMemoryUniquenessProvider                                node/.../transactions/InMemoryUniquenessProvider.kt
  PersistentUniquenessProvider (RDBMS, ThreadBox-locked)    node/.../transactions/PersistentUniquenessProvider.kt:19-81
    committedStates: StateRef -> ConsumingTx(id, inputIndex, requestingParty), table
    "node_notary_commit_log"; commit: under the lock, collect every input already in the map (in
    input order) -> UniquenessException(Conflict(those)); otherwise put(state, ConsumingTx(txId, i,
    caller)) for every input (a repeated input is re-put: the last index wins).

`commit_batch(requests)` is the batched commit of a verified notary batch: the requests are decided
in request order, exactly as that many sequential `commit` calls would decide them (a request
conflicts with states committed by an EARLIER request of the same batch, never a later one, and a
conflicting request commits nothing), but the persistent provider does it in ONE database
transaction — one lock acquisition and one durable commit (fsync) per batch instead of per
transaction.  Each result is None (committed) or the UniquenessConflict the sequential call would
have raised.  DeviceUniquenessProvider makes the same decisions on the GPU: the device-resident set of
include/cordaverify.h (cv_uniq), one call per batch, optionally with the persistent provider as its durable log.
Its snapshot() / install() are DistributedImmutableMap's (the Raft notary's state machine, corda_amd/raft.py): a
Snapshot carries the set's entries and the party table, and goes to a file and back.

The node's JDBC/H2 store is out of scope; the persistent provider keeps the
reference's table and columns on SQLite (Python's sqlite3, synchronous=FULL, WAL journal), keyed by
the canonical encoding of the state reference.
"""
from __future__ import annotations

import hashlib
import sqlite3
import struct
import threading
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .crypto import IllegalArgumentException
from .transactions import SecureHash


@dataclass(frozen=True)
class ConsumingTx:
    """UniquenessProvider.ConsumingTx(id, inputIndex, requestingParty) (UniquenessProvider.kt:31)."""
    id: SecureHash
    input_index: int
    requesting_party: str


def _enc(x) -> bytes:
    """Canonical tagged encoding of the state references and parties a conflict report carries and
    the persistent provider keys its rows by (the reference's Kryo serialization is out of scope)."""
    if isinstance(x, SecureHash):
        return b"H" + x.bytes
    if isinstance(x, (bytes, bytearray)):
        return b"B" + struct.pack("<I", len(x)) + bytes(x)
    if isinstance(x, str):
        b = x.encode()
        return b"S" + struct.pack("<I", len(b)) + b
    if isinstance(x, bool) or not isinstance(x, (int, tuple, list)):
        raise IllegalArgumentException(f"cannot serialize {type(x).__name__}")
    if isinstance(x, int):
        return b"I" + struct.pack("<q", x)
    return b"T" + struct.pack("<I", len(x)) + b"".join(_enc(v) for v in x)


def _dec(b: bytes, p: int):
    t = b[p:p + 1]
    p += 1
    if t == b"H":
        return SecureHash(b[p:p + 32]), p + 32
    if t in (b"B", b"S"):
        (m,) = struct.unpack_from("<I", b, p)
        v = b[p + 4:p + 4 + m]
        return (bytes(v) if t == b"B" else v.decode()), p + 4 + m
    if t == b"I":
        return struct.unpack_from("<q", b, p)[0], p + 8
    if t == b"T":
        (m,) = struct.unpack_from("<I", b, p)
        p += 4
        out = []
        for _ in range(m):
            v, p = _dec(b, p)
            out.append(v)
        return tuple(out), p
    raise IllegalArgumentException("malformed conflict encoding")


@dataclass
class UniquenessConflict:
    """UniquenessProvider.Conflict(stateHistory): the consuming transaction of every conflicting state."""
    state_history: Dict[object, ConsumingTx]

    def serialize(self) -> bytes:
        rows = sorted((_enc(s), c) for s, c in self.state_history.items())
        return b"CONFLICT" + _enc(tuple((s_enc, c.id, c.input_index, c.requesting_party) for s_enc, c in rows))

    @staticmethod
    def deserialize(raw: bytes) -> "UniquenessConflict":
        if not raw.startswith(b"CONFLICT"):
            raise IllegalArgumentException("not a conflict report")
        rows, _ = _dec(raw, 8)
        return UniquenessConflict({_dec(s_enc, 0)[0]: ConsumingTx(h, i, party) for s_enc, h, i, party in rows})


class UniquenessException(Exception):
    """UniquenessException(error: Conflict) (UniquenessProvider.kt:34)."""

    def __init__(self, conflict: UniquenessConflict):
        super().__init__("conflict")
        self.error = conflict


CommitRequest = Tuple[Sequence[object], SecureHash, str]     # (input states, tx id, caller identity)


class InMemoryUniquenessProvider:
    """InMemoryUniquenessProvider.kt semantics: all-or-nothing commit under one lock."""

    def __init__(self):
        self.committed: Dict[object, ConsumingTx] = {}
        self._lock = threading.Lock()

    def _commit_locked(self, states, tx_id, caller) -> Optional[UniquenessConflict]:
        conflict = {s: self.committed[s] for s in states if s in self.committed}
        if conflict:
            return UniquenessConflict(conflict)
        for i, s in enumerate(states):
            self.committed[s] = ConsumingTx(tx_id, i, caller)
        return None

    def commit(self, states: Sequence[object], tx_id: SecureHash, caller: str) -> None:
        with self._lock:
            c = self._commit_locked(states, tx_id, caller)
        if c is not None:
            raise UniquenessException(c)

    def commit_batch(self, requests: Sequence[CommitRequest]) -> List[Optional[UniquenessConflict]]:
        with self._lock:
            return [self._commit_locked(s, t, c) for s, t, c in requests]


class PersistentUniquenessProvider:
    """PersistentUniquenessProvider.kt:19-81 on SQLite: table node_notary_commit_log, one row per
    consumed state (state reference -> consuming transaction id, input index, requesting party).
    Thread-safe (one connection behind a lock, as the reference's ThreadBox); every commit or batch
    is one IMMEDIATE transaction, durable when it returns (synchronous=FULL)."""

    TABLE = "node_notary_commit_log"

    def __init__(self, path: str):
        self.path = path
        self._lock = threading.Lock()
        self._db = sqlite3.connect(path, isolation_level=None, check_same_thread=False)
        self._db.execute("PRAGMA journal_mode=WAL")
        self._db.execute("PRAGMA synchronous=FULL")
        self._db.execute(f"CREATE TABLE IF NOT EXISTS {self.TABLE} ("
                         "output BLOB PRIMARY KEY, consuming_transaction_id BLOB NOT NULL, "
                         "consuming_input_index INTEGER NOT NULL, requesting_party_name TEXT NOT NULL)")

    def close(self) -> None:
        with self._lock:
            self._db.close()

    def __len__(self) -> int:
        with self._lock:
            return self._db.execute(f"SELECT COUNT(*) FROM {self.TABLE}").fetchone()[0]

    def get(self, state) -> Optional[ConsumingTx]:
        with self._lock:
            r = self._db.execute(f"SELECT consuming_transaction_id, consuming_input_index, requesting_party_name "
                                 f"FROM {self.TABLE} WHERE output = ?", (_enc(state),)).fetchone()
        return None if r is None else ConsumingTx(SecureHash(bytes(r[0])), int(r[1]), r[2])

    def _lookup(self, keys: List[bytes]) -> Dict[bytes, ConsumingTx]:
        found: Dict[bytes, ConsumingTx] = {}
        for j in range(0, len(keys), 500):                  # SQLite's bound-parameter limit
            part = keys[j:j + 500]
            q = (f"SELECT output, consuming_transaction_id, consuming_input_index, requesting_party_name "
                 f"FROM {self.TABLE} WHERE output IN ({','.join('?' * len(part))})")
            for out, h, i, party in self._db.execute(q, part):
                found[bytes(out)] = ConsumingTx(SecureHash(bytes(h)), int(i), party)
        return found

    def _decide(self, requests: Sequence[CommitRequest]) -> Tuple[List[Optional[UniquenessConflict]], list]:
        """Sequential decisions of the batch against the store plus the batch's own earlier commits."""
        keyed = [[_enc(s) for s in states] for states, _, _ in requests]
        stored = self._lookup(sorted({k for ks in keyed for k in ks}))
        pending: Dict[bytes, ConsumingTx] = {}
        out: List[Optional[UniquenessConflict]] = []
        rows = []
        for (states, tx_id, caller), ks in zip(requests, keyed):
            conflict = {}
            for s, k in zip(states, ks):
                c = pending.get(k) or stored.get(k)
                if c is not None:
                    conflict[s] = c
            if conflict:
                out.append(UniquenessConflict(conflict))
                continue
            for i, k in enumerate(ks):                      # put(): a repeated input is re-put, last index wins
                pending[k] = ConsumingTx(tx_id, i, caller)
            rows.extend((k, tx_id.bytes, i, caller) for i, k in enumerate(ks))
            out.append(None)
        return out, rows

    def commit_batch(self, requests: Sequence[CommitRequest]) -> List[Optional[UniquenessConflict]]:
        with self._lock:
            self._db.execute("BEGIN IMMEDIATE")
            try:
                out, rows = self._decide(requests)
                self._db.executemany(f"INSERT OR REPLACE INTO {self.TABLE} VALUES (?, ?, ?, ?)", rows)
                self._db.execute("COMMIT")
            except BaseException:
                # a failed COMMIT (disk / fsync error) may already have rolled back: a second ROLLBACK
                # would raise "no transaction is active" and replace the error the notary must report
                if self._db.in_transaction:
                    try:
                        self._db.execute("ROLLBACK")
                    except Exception:  # noqa: BLE001 - the original exception is the one to report
                        pass
                raise
        return out

    def commit(self, states: Sequence[object], tx_id: SecureHash, caller: str) -> None:
        (c,) = self.commit_batch([(states, tx_id, caller)])
        if c is not None:
            raise UniquenessException(c)


@dataclass(eq=False)
class Snapshot:
    """The contents of a DeviceUniquenessProvider at one moment: the party table and the four arrays of
    native.UniquenessSet.snapshot (state_key (n,32) u8, consumed_id (n,32) u8, consumed_index u32[n], consumed_caller
    u32[n]).  consumed_caller holds handles into `parties`, so the arrays mean nothing without the table.

    write / read: one file — magic "CVUSNAP1", u32 version, u32 flags (bit 0: leaf_keys), u64 entries, u32 parties;
    each party name as u32 length + UTF-8; the four arrays, little-endian, in the order above; the SHA-256 of
    everything before it.  read refuses a file whose trailer, magic, version or length is wrong."""
    parties: List[str]
    state_key: np.ndarray
    consumed_id: np.ndarray
    consumed_index: np.ndarray
    consumed_caller: np.ndarray
    leaf_keys: bool = False

    MAGIC = b"CVUSNAP1"
    VERSION = 1

    def __len__(self) -> int:
        return int(self.consumed_index.shape[0])

    def arrays(self):
        return self.state_key, self.consumed_id, self.consumed_index, self.consumed_caller

    def to_bytes(self) -> bytes:
        n = len(self)
        names = [p.encode() for p in self.parties]
        body = b"".join([self.MAGIC, struct.pack("<IIQI", self.VERSION, 1 if self.leaf_keys else 0, n, len(names)),
                         b"".join(struct.pack("<I", len(b)) + b for b in names),
                         np.ascontiguousarray(self.state_key, np.uint8).tobytes(),
                         np.ascontiguousarray(self.consumed_id, np.uint8).tobytes(),
                         np.ascontiguousarray(self.consumed_index, "<u4").tobytes(),
                         np.ascontiguousarray(self.consumed_caller, "<u4").tobytes()])
        return body + hashlib.sha256(body).digest()

    @classmethod
    def from_bytes(cls, raw: bytes) -> "Snapshot":
        bad = IllegalArgumentException
        if len(raw) < len(cls.MAGIC) + 20 + 32 or raw[:8] != cls.MAGIC:
            raise bad("not a uniqueness snapshot")
        if hashlib.sha256(raw[:-32]).digest() != raw[-32:]:
            raise bad("uniqueness snapshot: the SHA-256 trailer does not match")
        version, flags, n, nparties = struct.unpack_from("<IIQI", raw, 8)
        if version != cls.VERSION:
            raise bad(f"uniqueness snapshot: version {version}")
        p, end = 28, len(raw) - 32
        parties = []
        for _ in range(nparties):
            if p + 4 > end:
                raise bad("uniqueness snapshot: truncated party table")
            (m,) = struct.unpack_from("<I", raw, p)
            if p + 4 + m > end:
                raise bad("uniqueness snapshot: truncated party table")
            parties.append(raw[p + 4:p + 4 + m].decode())
            p += 4 + m
        if end - p != 72 * n:
            raise bad("uniqueness snapshot: the arrays do not fill the file")
        key = np.frombuffer(raw, np.uint8, 32 * n, p).reshape(n, 32).copy()
        cid = np.frombuffer(raw, np.uint8, 32 * n, p + 32 * n).reshape(n, 32).copy()
        cix = np.frombuffer(raw, "<u4", n, p + 64 * n).astype(np.uint32)
        cc = np.frombuffer(raw, "<u4", n, p + 68 * n).astype(np.uint32)
        if n and int(cc.max()) >= nparties:
            raise bad("uniqueness snapshot: a caller handle past the party table")
        return cls(parties, key, cid, cix, cc, bool(flags & 1))

    def write(self, path: str) -> None:
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @classmethod
    def read(cls, path: str) -> "Snapshot":
        with open(path, "rb") as f:
            return cls.from_bytes(f.read())


class DeviceUniquenessProvider:
    """The commit step on the device: a native.UniquenessSet (cv_uniq, include/cordaverify.h) behind the interface
    of the two providers above.  A batch is decided in ONE call, exactly as InMemoryUniquenessProvider.commit_batch
    decides it.

    The set's key is sha256(_enc(state)) (the reference's choice would be SecureHash.sha256 of the serialised
    StateRef, Structures.kt:337); party names map to u32 handles through a table kept here; a conflict comes back
    as the UniquenessConflict the sequential call would have raised.  The set grows (reserve) when a batch would
    pass its capacity.

    The device set is not durable.  With log= a PersistentUniquenessProvider, the set is loaded from the log's rows
    at start, and each batch's accepted rows are appended to the log in one durable transaction before the call
    returns — no SELECT: the device has already decided.  If that append fails the error is raised and the provider
    refuses further work: the set then holds states the log does not, and has to be rebuilt from the log.

    leaf_keys=True keys the set by the SHA-256 of the raw state bytes — for a notary whose states are the serialised
    input leaves that is the input's Merkle leaf hash, the C-ABI's documented key (include/cordaverify.h, cv_uniq) and
    the one cv_notarise_batch takes from the leaf hashes on the device.  States must then be bytes.  The fused notary
    (notary.BatchingNotary(fused=True)) needs such a provider and drives it through fused(): the party handles, room
    reserved before the call, and the log append of the accepted rows."""

    def __init__(self, engine, capacity: int = 1 << 16, log: Optional[PersistentUniquenessProvider] = None,
                 leaf_keys: bool = False):
        from . import native
        self.leaf_keys = bool(leaf_keys)
        self._lock = threading.Lock()
        self._parties: List[str] = []
        self._handle: Dict[str, int] = {}
        self._log = log
        self._broken = False
        rows = []
        if log is not None:
            with log._lock:
                rows = log._db.execute(f"SELECT output, consuming_transaction_id, consuming_input_index, "
                                       f"requesting_party_name FROM {log.TABLE}").fetchall()
        self._set = native.UniquenessSet(engine, max(int(capacity), 2 * len(rows), 1))
        if rows:
            self._set.load(np.frombuffer(b"".join(self._row_key(bytes(r[0])) for r in rows), np.uint8),
                           np.frombuffer(b"".join(bytes(r[1]) for r in rows), np.uint8),
                           np.array([int(r[2]) for r in rows], np.uint32),
                           np.array([self._party(r[3]) for r in rows], np.uint32))

    @staticmethod
    def _key(enc: bytes) -> bytes:
        return hashlib.sha256(enc).digest()

    def _state_key(self, state, enc: bytes) -> bytes:
        if not self.leaf_keys:
            return self._key(enc)
        if not isinstance(state, (bytes, bytearray)):
            raise TypeError("leaf_keys: a state is the bytes of its serialised input leaf")
        return hashlib.sha256(bytes(state)).digest()

    def _row_key(self, enc: bytes) -> bytes:
        """The set's key of a log row (the log stores _enc(state))."""
        return self._state_key(_dec(enc, 0)[0], enc) if self.leaf_keys else self._key(enc)

    def _append(self, rows) -> None:
        """The accepted rows (_enc(state), tx id bytes, input index, caller name) into the log, in one durable
        transaction; a failure marks the provider broken (the set is then ahead of its log).  Caller holds the lock."""
        if self._log is None:
            return
        try:
            with self._log._lock:
                db = self._log._db
                db.execute("BEGIN IMMEDIATE")
                try:
                    db.executemany(f"INSERT OR REPLACE INTO {self._log.TABLE} VALUES (?, ?, ?, ?)", rows)
                    db.execute("COMMIT")
                except BaseException:
                    if db.in_transaction:
                        try:
                            db.execute("ROLLBACK")
                        except Exception:  # noqa: BLE001 - the original exception is the one to report
                            pass
                    raise
        except BaseException:
            self._broken = True
            raise

    def fused(self, callers: Sequence[str], nstates: int, call):
        """What notary.BatchingNotary(fused=True) needs around ONE cv_notarise_batch, under the provider's lock: the
        callers' party handles, room for nstates more states reserved beforehand, then call(uniqueness set, handles)
        -> (result, accepted rows for the log), the rows appended durably before the result is released.  Returns
        (result, party names by handle)."""
        with self._lock:
            if self._broken:
                raise RuntimeError("the device set is ahead of its log: rebuild it from the log")
            handles = np.array([self._party(c) for c in callers], np.uint32)
            st = self._set.stats()
            if st["resident"] + nstates > st["capacity"]:
                self._set.reserve(max(2 * st["capacity"], st["resident"] + nstates))
            result, rows = call(self._set, handles)
            self._append([(_enc(s), t, i, c) for s, t, i, c in rows])
            return result, list(self._parties)

    def _party(self, name: str) -> int:
        h = self._handle.get(name)
        if h is None:
            h = self._handle[name] = len(self._parties)
            self._parties.append(name)
        return h

    def close(self) -> None:
        self._set.close()

    def __len__(self) -> int:
        return self._set.stats()["resident"]

    def snapshot(self, max_entries: Optional[int] = None) -> Snapshot:
        """DistributedImmutableMap.snapshot (DistributedImmutableMap.kt:87-92): every entry of the set with the party
        table its caller handles index, read out of device memory in one pass (chunked when max_entries is given)."""
        with self._lock:
            key, cid, cix, cc = self._set.snapshot(max_entries)
            return Snapshot(list(self._parties), key, cid, cix, cc, self.leaf_keys)

    def install(self, snapshot: Snapshot) -> None:
        """DistributedImmutableMap.install (DistributedImmutableMap.kt:95-105): the set's contents and the party
        table become the snapshot's.  A provider with a log keeps to its log: the set stores key hashes, not the state
        references the log's rows are keyed by, so a log cannot be rebuilt from a snapshot."""
        if self._log is not None:
            raise IllegalArgumentException("install: this provider is warmed from its commit log")
        if bool(snapshot.leaf_keys) != self.leaf_keys:
            raise IllegalArgumentException("install: the snapshot's keys are of the other kind (leaf_keys)")
        if len(snapshot) and int(snapshot.consumed_caller.max()) >= len(snapshot.parties):
            raise IllegalArgumentException("install: a caller handle past the party table")
        with self._lock:
            self._set.install(*snapshot.arrays())
            self._parties = list(snapshot.parties)
            self._handle = {name: h for h, name in enumerate(self._parties)}

    def get(self, state) -> Optional[ConsumingTx]:
        with self._lock:
            found, cid, cix, cc = self._set.lookup(np.frombuffer(self._state_key(state, _enc(state)), np.uint8))
            return ConsumingTx(SecureHash(cid[0].tobytes()), int(cix[0]), self._parties[int(cc[0])]) if found[0] else None

    def commit_batch(self, requests: Sequence[CommitRequest]) -> List[Optional[UniquenessConflict]]:
        if not requests:
            return []
        encs = [[_enc(s) for s in states] for states, _, _ in requests]
        begin = np.zeros(len(requests) + 1, np.uint32)
        np.cumsum([len(e) for e in encs], out=begin[1:])
        ns = int(begin[-1])
        keys = np.frombuffer(b"".join(self._state_key(s, e) for (states, _, _), es in zip(requests, encs)
                                      for s, e in zip(states, es)), np.uint8)
        ids = np.frombuffer(b"".join(t.bytes for _, t, _ in requests), np.uint8)
        with self._lock:
            if self._broken:
                raise RuntimeError("the device set is ahead of its log: rebuild it from the log")
            callers = np.array([self._party(c) for _, _, c in requests], np.uint32)
            st = self._set.stats()
            if st["resident"] + ns > st["capacity"]:
                self._set.reserve(max(2 * st["capacity"], st["resident"] + ns))
            status, conflict, cid, cix, cc = self._set.commit_batch(keys, begin, ids, callers)
            if self._log is not None:
                self._append([(e, t.bytes, i, c) for (_, t, c), es, ok in zip(requests, encs, status == 0) if ok
                              for i, e in enumerate(es)])
            parties = list(self._parties)
        out: List[Optional[UniquenessConflict]] = []
        for t, (states, _, _) in enumerate(requests):
            if status[t] == 0:
                out.append(None)
                continue
            b = int(begin[t])
            out.append(UniquenessConflict({s: ConsumingTx(SecureHash(cid[b + j].tobytes()), int(cix[b + j]),
                                                          parties[int(cc[b + j])])
                                           for j, s in enumerate(states) if conflict[b + j]}))
        return out

    def commit(self, states: Sequence[object], tx_id: SecureHash, caller: str) -> None:
        (c,) = self.commit_batch([(states, tx_id, caller)])
        if c is not None:
            raise UniquenessException(c)
