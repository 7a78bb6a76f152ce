"""CPU: the guard-band arena (tests/guard_arena.py) against stand-in "calls" written in numpy: what check_untouched must report,
what it must let pass, the alignment of the placements and the two poisons."""
import numpy as np
import pytest

import guard_arena as ga


def layout(poison, align=4, n=1001):
    """one call's buffers: float input, label input with a label cycle in its guards, two outputs"""
    rng = np.random.default_rng(1)
    a = ga.Arena(poison, capacity=1 << 20)
    x = a.place(rng.normal(size=(n, 3)).astype(np.float32), max(align, 4), "in", name="x")
    labels = a.place(np.arange(n, dtype=np.uint32) + 7, max(align, 4), "in", guard=np.arange(5, dtype=np.uint32) + 2000, name="labels")
    out = a.place(np.empty(n, np.float32), max(align, 4), "out", name="out")
    codes = a.place(np.empty((n, 3), np.uint8), align, "out", name="codes")
    return a, x, labels, out, codes


def call(x, labels, out, codes):
    out[:] = x.sum(1) + labels
    codes[:] = (labels[:, None] + np.arange(3)) & 0x7F


def flat(a):
    return a.buf                                            # the stand-in for a pointer that strays: the arena's own bytes


@pytest.mark.parametrize("poison", ga.POISONS)
def test_a_call_that_writes_only_its_outputs_passes(poison):
    a, x, labels, out, codes = layout(poison)
    a.snapshot()
    call(x, labels, out, codes)
    a.check_untouched([out, codes])
    assert np.array_equal(a.host(codes), (labels[:, None] + np.arange(3)) & 0x7F)
    with pytest.raises(ga.GuardError, match="outside its declared part"):
        a.check_untouched([out])                            # codes was written and is not declared


@pytest.mark.parametrize("poison", ga.POISONS)
@pytest.mark.parametrize("where", ["before", "after"])
@pytest.mark.parametrize("which", ["out", "codes"])
def test_a_write_one_byte_outside_an_output_is_reported(poison, where, which):
    a, x, labels, out, codes = layout(poison)
    a.snapshot()
    call(x, labels, out, codes)
    p = a._placement(out if which == "out" else codes)
    at = p.off - 1 if where == "before" else p.off + p.nbytes
    flat(a)[at] ^= 0x21
    with pytest.raises(ga.GuardError, match=("1 bytes in front of %s" if where == "before" else "1 bytes behind the end of %s") % which):
        a.check_untouched([out, codes])


@pytest.mark.parametrize("poison", ga.POISONS)
def test_a_write_into_an_input_is_reported(poison):
    a, x, labels, out, codes = layout(poison)
    a.snapshot()
    call(x, labels, out, codes)
    labels[-1] += 1
    with pytest.raises(ga.GuardError, match="of labels \\(input\\)"):
        a.check_untouched([out, codes])
    with pytest.raises(ValueError):
        a.check_untouched([out, codes, labels])             # an input cannot be declared an output


@pytest.mark.parametrize("poison", ga.POISONS)
def test_a_declared_prefix_and_a_refused_call(poison):
    a, x, labels, out, codes = layout(poison)
    a.snapshot()
    a.check_untouched([])                                   # a refused call writes nothing
    out[:994] = 1.0
    a.check_untouched([(out, 994)])                         # capacity 7 over: the tail stays
    image = a.host(out)[994:].view(np.uint8)
    assert (image == (ga.P1_BYTE if poison == ga.P1 else ga.P2_OUT_BYTE)).all()
    out[994] = 1.0
    with pytest.raises(ga.GuardError, match="byte 3976 of out"):
        a.check_untouched([(out, 994)])
    with pytest.raises(ValueError):
        a.check_untouched([(out, 1002)])


@pytest.mark.parametrize("align", [1, 2, 4, 8, 16, 256])
def test_placements_have_exactly_the_alignment_asked_for(align):
    a = ga.Arena(ga.P1, capacity=2 << 20)
    for n in (1, 3, 1001, 4096):
        v = a.place(np.zeros(n, np.uint8 if align < 4 else np.float32), align, "in")
        addr = a.ptr(v)
        assert addr == v.ctypes.data and addr % align == 0 and addr % (2 * align) == align
    offs = [(p.lead, p.off, p.off + p.nbytes, p.end) for p in a.placed]
    for lead, off, stop, end in offs:
        assert off - lead >= ga.GUARD and end - stop == ga.GUARD and off - lead < ga.GUARD + 2 * align
    assert offs[0][0] == 0 and all(offs[i][3] == offs[i + 1][0] for i in range(len(offs) - 1))   # no byte belongs to nobody


def test_the_two_poisons_differ_in_every_guard_byte_and_every_output_byte():
    (a1, *v1), (a2, *v2) = layout(ga.P1), layout(ga.P2)
    m1, b1 = a1.guards()
    m2, b2 = a2.guards()
    assert (b1[m1] == 0xFF).all() and (b2[m2] != 0xFF).all() and m1.sum() >= 8 * ga.GUARD
    assert (a1.host(v1[2]).view(np.uint8) == 0xFF).all() and (a2.host(v2[2]).view(np.uint8) == 0x5A).all()
    # P2 lays the label cycle so that the elements next to the buffer are whole labels the "index" holds
    p = a2._placement(v2[1])
    around = b2[p.off - 40:p.off].view(np.uint32).tolist() + b2[p.off + p.nbytes:p.off + p.nbytes + 40].view(np.uint32).tolist()
    assert set(around) == set(range(2000, 2005))
    assert (b2[a2._placement(v2[0]).off - 64:a2._placement(v2[0]).off] == 0).all()                 # float guards: zeros
    with pytest.raises(ValueError):
        a2.place(np.zeros(4, np.uint32), 4, "in", guard=np.array([0x12FF], np.uint32))


def test_a_stray_read_changes_the_answer_under_one_poison_at_least():
    """the stand-in reads one label past n: the outputs of the two poisons differ, which is how property R sees it"""
    got = []
    for poison in ga.POISONS:
        a, x, labels, out, codes = layout(poison)
        p = a._placement(labels)
        stray = flat(a)[p.off:p.off + p.nbytes + 4].view(np.uint32)                                # n + 1 labels
        got.append(int(stray.astype(np.uint64).sum()))
    assert got[0] != got[1] and got[1] - int((np.arange(1001) + 7).sum()) in range(2000, 2005)
