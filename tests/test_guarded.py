"""tests/guarded.py on host memory: the placement rule, the poison, and that check_guards names the byte that
changed — a guard check that cannot fail would make the output-contract tests vacuous."""
import numpy as np
import pytest

from guarded import GUARD, Guarded, GuardError, corpus_rows, tail_bits


def _g(fill=0xA5):
    return Guarded([("bitmap", 24, 8), ("status", 5, 1), ("ids", 64, 16), ("words", 12, 4)], fill)


def test_placement_and_poison():
    g = _g()
    for name, (off, nbytes, align) in g.slots.items():
        a = g.ptr(name)
        assert a % align == 0 and a % (2 * align) == align, name
        assert g.untouched(name) and g.read(name).size == nbytes
    ends = [0] + [off + nb for off, nb, _ in g.slots.values()]
    starts = [off for off, _, _ in g.slots.values()] + [g.total]
    assert all(s - e >= GUARD for s, e in zip(starts, ends))
    assert g.first_changed_guard() is None
    g.check_guards()


@pytest.mark.parametrize("name,where,offset", [("bitmap", "after", 0), ("bitmap", "before", 1), ("status", "after", 7),
                                               ("ids", "before", 3), ("words", "after", GUARD - 1)])
def test_a_changed_guard_byte_is_named(name, where, offset):
    g = _g(0x00)
    off, nbytes, _ = g.slots[name]
    g.buf[off + nbytes + offset if where == "after" else off - offset] = 0x80
    assert g.first_changed_guard() == (name, where, offset, 0x80)
    with pytest.raises(GuardError, match=f"guard byte {offset} {where} output '{name}'"):
        g.check_guards("case")
    g.refill()
    g.check_guards()


def test_writes_inside_an_output_are_not_guard_changes():
    g = _g(0xFF)
    off, nbytes, _ = g.slots["ids"]
    g.buf[off:off + nbytes] = 0
    g.check_guards()
    assert not g.untouched("ids") and g.untouched("status")
    assert g.read("ids", np.uint32, (4, 4)).shape == (4, 4)


def test_corpus_rows_and_tail_bits(corpus):
    for n in (1, 2, 65, 513, 4097):
        for last in ("accepted", "bad_key"):
            rows = corpus_rows(corpus, n, last)
            assert len(rows) == n and np.array_equal(rows, corpus_rows(corpus, n, last))
            assert len(set(rows[:min(n, len(corpus["pk"]))].tolist())) == min(n, len(corpus["pk"]))
            assert (corpus["verdict"][rows[-1]] == 1) == (last == "accepted")
    assert tail_bits(np.array([0x1F], np.uint64), 5) == 0 and tail_bits(np.array([0x3F], np.uint64), 5) == 1
    assert tail_bits(np.array([7, 1 << 63], np.uint64), 128) == 0
