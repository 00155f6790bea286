"""The registry of derived weight copies, the gradient arena and the layer selection of the step plan, on CPU tensors."""
import gc
import math
import weakref

import torch
import torch.nn as nn

from feature_intertwiner_amd import step_state as S


def _weight(*shape):
    return torch.randn(*(shape or (8, 4, 1, 1)))


def test_a_copy_is_returned_for_the_owner_and_for_its_aliases():
    reg, w = S.Registry(), torch.randn(8, 16, 3, 3).contiguous(memory_format=torch.channels_last)
    wt, fr, lo = torch.empty(16, 3, 3, 8), torch.empty(128), torch.empty(w.numel(), dtype=torch.bfloat16)
    reg.publish(w, S.WT, wt, (False, tuple(w.shape)))
    reg.publish(w, S.FRAG, fr, (8, 16))
    reg.publish(w, S.LOWP, lo, (torch.bfloat16, w.numel()))
    assert len(reg.table) == 1
    view = w.permute(0, 2, 3, 1)                    # what _conv_fwd makes of a channels-last parameter
    assert view.data_ptr() == w.data_ptr() and view.is_contiguous()
    for alias in (w, w.detach(), view):
        assert reg.lookup(alias, S.FRAG, (8, 16)) is fr
        assert reg.lookup(alias, S.LOWP, (torch.bfloat16, w.numel())) is lo
    assert reg.lookup(w.detach(), S.WT, (False, tuple(w.shape))) is wt


def test_a_copy_is_void_after_an_in_place_write():
    reg, w = S.Registry(), _weight()
    reg.publish(w, S.FRAG, torch.empty(32), (8, 4))
    assert reg.lookup(w, S.FRAG, (8, 4)) is not None
    w.add_(0)
    assert reg.lookup(w, S.FRAG, (8, 4)) is None
    assert reg.lookup(w.detach(), S.FRAG, (8, 4)) is None


def test_a_copy_is_void_once_its_owner_is_gone_though_the_address_lives_on():
    """The address-reuse failure without allocator luck: the alias keeps storage, address and version counter."""
    reg, w = S.Registry(), _weight()
    alias = w.detach()
    reg.publish(w, S.FRAG, torch.empty(32), (8, 4))
    key, version = w.data_ptr(), w._version
    assert reg.lookup(alias, S.FRAG, (8, 4)) is not None
    del w
    gc.collect()
    rec = reg.table[key]
    assert rec.owner() is None and alias.data_ptr() == key and rec.version == version == alias._version
    assert reg.lookup(alias, S.FRAG, (8, 4)) is None


def test_a_copy_is_void_once_its_owner_has_moved():
    reg, w = S.Registry(), torch.nn.Parameter(torch.randn(8, 16, 3, 3))
    alias = w.detach()
    reg.publish(w, S.LOWP, torch.empty(w.numel(), dtype=torch.float16), (torch.float16, w.numel()))
    w.data = w.data.contiguous(memory_format=torch.channels_last)       # the parameter now lives elsewhere
    assert reg.lookup(alias, S.LOWP, (torch.float16, alias.numel())) is None


def test_a_copy_is_void_for_another_expectation():
    reg, w = S.Registry(), _weight(8, 4, 1, 1)
    reg.publish(w, S.WT, torch.empty(4, 1, 1, 8), (True, (8, 4, 1, 1)))
    reg.publish(w, S.FRAG, torch.empty(32), (8, 4))
    reg.publish(w, S.LOWP, torch.empty(32, dtype=torch.bfloat16), (torch.bfloat16, 32))
    assert reg.lookup(w, S.WT, (True, (8, 4, 1, 1))) is not None
    assert reg.lookup(w, S.WT, (False, (8, 4, 1, 1))) is None
    assert reg.lookup(w, S.FRAG, (4, 8)) is None
    assert reg.lookup(w, S.LOWP, (torch.float16, 32)) is None
    assert reg.lookup(w[:4], S.LOWP, (torch.bfloat16, 16)) is None      # a narrower view at the same address
    other = _weight()
    assert reg.lookup(other, S.FRAG, (8, 4)) is None


def test_a_record_republished_with_its_source_ignores_the_version_until_the_source_is_republished():
    reg, w, wt = S.Registry(), _weight(8, 4, 1, 1), torch.empty(4, 1, 1, 8)
    reg.publish(w, S.WT, wt, (False, (8, 4, 1, 1)))
    fr, lo = torch.empty(32), torch.empty(32, dtype=torch.bfloat16)
    reg.publish(wt, S.FRAG, fr, (4, 8), with_source=True)
    reg.publish(wt, S.LOWP, lo, (torch.bfloat16, 32), with_source=True)
    assert reg.table[wt.data_ptr()].version is S.WITH_SOURCE
    wt.add_(0)                                      # (the batched transpose does not even do that)
    assert reg.lookup(wt, S.FRAG, (4, 8)) is fr and reg.lookup(wt, S.LOWP, (torch.bfloat16, 32)) is lo
    w.add_(0)
    reg.publish(w, S.WT, wt, (False, (8, 4, 1, 1)))         # W^T rewritten in place: what was derived from it is gone
    assert reg.lookup(w, S.WT, (False, (8, 4, 1, 1))) is wt
    assert reg.lookup(wt, S.FRAG, (4, 8)) is None and reg.lookup(wt, S.LOWP, (torch.bfloat16, 32)) is None
    assert wt.data_ptr() not in reg.table


def test_publishing_at_a_new_version_drops_the_copies_of_the_old_one():
    reg, w = S.Registry(), _weight(8, 4, 1, 1)
    reg.publish(w, S.LOWP, torch.empty(32, dtype=torch.bfloat16), (torch.bfloat16, 32))
    w.add_(0)
    reg.publish(w, S.FRAG, torch.empty(32), (8, 4))
    assert reg.lookup(w, S.FRAG, (8, 4)) is not None
    assert reg.lookup(w, S.LOWP, (torch.bfloat16, 32)) is None
    assert S.LOWP not in reg.table[w.data_ptr()].copies


def test_sweep_removes_exactly_the_dead_owner_records_and_keeps_pinned_temporaries():
    reg = S.Registry()
    live, dead, temp = _weight(), _weight(), _weight()
    reg.publish(live, S.FRAG, torch.empty(32), (8, 4))
    reg.publish(dead, S.FRAG, torch.empty(32), (8, 4))
    reg.publish(temp, S.LOWP, torch.empty(32, dtype=torch.bfloat16), (torch.bfloat16, 32), pinned=True)
    keys = (live.data_ptr(), dead.data_ptr(), temp.data_ptr())
    ref = weakref.ref(temp)
    del dead, temp
    gc.collect()
    assert ref() is not None                        # the record pins the temporary: its address cannot be reused
    reg.sweep()
    assert set(reg.table) == {keys[0], keys[2]}
    assert reg.table[keys[2]].pin is not None and reg.table[keys[0]].pin is None
    assert reg.lookup(ref(), S.LOWP, (torch.bfloat16, 32)) is not None
    reg.clear()
    assert not reg.table
    gc.collect()
    assert ref() is None


def test_sweep_follows_a_dead_weight_to_the_records_of_its_transpose():
    reg, w, wt = S.Registry(), _weight(8, 4, 1, 1), torch.empty(4, 1, 1, 8)
    reg.publish(w, S.WT, wt, (False, (8, 4, 1, 1)))
    reg.publish(wt, S.FRAG, torch.empty(32), (4, 8), with_source=True)
    keep = _weight()
    reg.publish(keep, S.FRAG, torch.empty(32), (8, 4))
    del w, wt                                       # the weight's record still holds W^T
    gc.collect()
    assert len(reg.table) == 3
    reg.sweep()
    assert set(reg.table) == {keep.data_ptr()}


def test_a_temporary_copy_of_a_transpose_does_not_outlive_its_republication():
    """A 16-bit copy made on the fly of a W^T (a call in a 16-bit precision under an fp32 plan) joins the W^T's record."""
    reg, w, wt = S.Registry(), _weight(8, 4, 1, 1), torch.empty(4, 1, 1, 8)
    reg.publish(w, S.WT, wt, (False, (8, 4, 1, 1)))
    fr = torch.empty(32)
    reg.publish(wt, S.FRAG, fr, (4, 8), with_source=True)
    reg.publish(wt, S.LOWP, wt.to(torch.bfloat16), (torch.bfloat16, 32), pinned=True)
    assert reg.lookup(wt, S.FRAG, (4, 8)) is fr and reg.lookup(wt, S.LOWP, (torch.bfloat16, 32)) is not None
    reg.publish(w, S.WT, wt, (False, (8, 4, 1, 1)))
    assert reg.lookup(wt, S.LOWP, (torch.bfloat16, 32)) is None
    reg.publish(wt, S.LOWP, wt.to(torch.bfloat16), (torch.bfloat16, 32), pinned=True)      # no record: pinned, versioned
    reg.publish(w, S.WT, wt, (False, (8, 4, 1, 1)))
    assert reg.lookup(wt, S.LOWP, (torch.bfloat16, 32)) is None


def test_the_bound_evicts_pinned_temporaries_only(monkeypatch):
    monkeypatch.setattr(S, "MAX_PINNED", 4)
    reg = S.Registry()
    owned = [_weight() for _ in range(6)]
    for w in owned:
        reg.publish(w, S.FRAG, torch.empty(32), (8, 4))
    temps = [_weight() for _ in range(4)]
    for t in temps:
        reg.publish(t, S.LOWP, torch.empty(32, dtype=torch.bfloat16), (torch.bfloat16, 32), pinned=True)
    reg.bound()
    assert len(reg.table) == 10                     # four pinned: at the bound, not past it
    extra = _weight()
    reg.publish(extra, S.LOWP, torch.empty(32, dtype=torch.bfloat16), (torch.bfloat16, 32), pinned=True)
    reg.bound()
    assert set(reg.table) == {w.data_ptr() for w in owned}
    assert all(reg.lookup(w, S.FRAG, (8, 4)) is not None for w in owned)


def test_temporaries_do_not_pile_up_across_republications():
    """A training step as conv._refresh_transposes runs it: release the temporaries, republish the weights; the backward
    pass then converts fresh temporaries.  The table stays at one step's worth."""
    reg = S.Registry()
    ws = [_weight(8, 4, 1, 1) for _ in range(3)]
    wts = [torch.empty(4, 1, 1, 8) for _ in ws]
    refs = []
    for step in range(50):
        reg.drop_pinned()
        for w, wt in zip(ws, wts):
            w.add_(0)
            reg.publish(w, S.WT, wt, (False, (8, 4, 1, 1)))
        for _ in range(4):
            t = _weight()
            reg.publish(t, S.LOWP, t.to(torch.bfloat16), (torch.bfloat16, 32), pinned=True)
            refs.append(weakref.ref(t))
        del t
        assert len(reg.table) == 3 + 4
        assert reg.pinned == {k for k, r in reg.table.items() if r.pin is not None} and len(reg.pinned) == 4
    gc.collect()
    assert sum(r() is not None for r in refs) == 4              # the fp32 sources of the earlier steps are free
    reg.drop_pinned()
    assert set(reg.table) == {w.data_ptr() for w in ws} and all(r.pin is None for r in reg.table.values())
    assert not reg.pinned
    assert all(reg.lookup(w, S.WT, (False, (8, 4, 1, 1))) is wt for w, wt in zip(ws, wts))


def test_clear_bumps_the_epoch():
    reg = S.Registry()
    reg.publish(_weight(), S.FRAG, torch.empty(32), (8, 4))
    e = reg.epoch
    reg.clear()
    assert not reg.table and reg.epoch == e + 1


def _armed(numel=40):
    arena, buf = S.GradArena(), torch.arange(float(numel))
    w, b, g = _weight(2, 3, 1, 1), torch.randn(2), torch.randn(4)
    slots = {("dw", w.data_ptr()): S.Slot(8, 6, weakref.ref(w), None),
             ("db", b.data_ptr()): S.Slot(16, 2, weakref.ref(b), None),
             ("bn", g.data_ptr()): S.Slot(20, 12, weakref.ref(g), b.data_ptr())}
    arena.arm(slots, buf)
    return arena, buf, w, b, g


def test_arena_take_hands_out_the_slot_and_says_whether_it_is_the_first_use():
    arena, buf, w, b, g = _armed()
    s, first = arena.take(("dw", w.data_ptr()), 6)
    assert first and s.data_ptr() == buf[8:].data_ptr() and torch.equal(s, torch.arange(8.0, 14.0))
    s2, first2 = arena.take(("dw", w.data_ptr()), 6)
    assert not first2 and s2.data_ptr() == s.data_ptr() and s2.numel() == 6
    s, first = arena.take(("bn", g.data_ptr()), 12, partner=b.data_ptr())
    assert first and torch.equal(s, torch.arange(20.0, 32.0))
    assert arena.take(("db", b.data_ptr()), 2, partner=12345)[1]         # a slot without a partner takes any
    arena.arm(arena.slots, buf)                                          # the next step: first uses again
    assert arena.take(("dw", w.data_ptr()), 6)[1]


def test_arena_take_gives_nothing_where_the_slot_is_not_this_tensors():
    arena, buf, w, b, g = _armed()
    none = (None, False)
    assert arena.take(("dw", w.data_ptr()), 5) == none                               # wrong numel
    assert arena.take(("dw", w.data_ptr() + 64), 6) == none                          # no slot
    assert arena.take(("bn", g.data_ptr()), 12, partner=b.data_ptr() + 4) == none    # laid out for another bias
    assert arena.take(("bn", g.data_ptr()), 12, partner=0) == none
    moved = torch.nn.Parameter(torch.randn(2, 3, 1, 1))
    key = ("dw", moved.data_ptr())
    arena.slots[key] = S.Slot(0, 6, weakref.ref(moved), None)
    assert arena.take(key, 6)[0] is not None
    moved.data = moved.data.clone()
    assert arena.take(key, 6) == none                                                # the owner lives elsewhere now
    key = ("dw", w.data_ptr())
    alias = w.detach()
    del w
    gc.collect()
    assert alias.data_ptr() == key[1] and arena.take(key, 6) == none                 # the owner is gone
    assert arena.take(("db", b.data_ptr()), 2)[0] is not None
    arena.disarm()
    assert arena.take(("db", b.data_ptr()), 2) == none
    arena.arm(arena.slots, None)                                                     # slots known, no cleared buffer
    assert arena.take(("db", b.data_ptr()), 2) == none


def test_the_plan_selects_layers_and_tile_bases_as_documented():
    from feature_intertwiner_amd import conv as C

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = C.Conv2d(3, 32, kernel_size=3, padding=1)              # Cin % 16 != 0
            self.c3 = C.Conv2d(32, 32, kernel_size=3, padding=1)
            self.bn3 = nn.BatchNorm2d(32)
            self.up = C.Conv2d(32, 128, kernel_size=1)
            self.c1 = C.Conv2d(128, 128, kernel_size=1)
            self.down = C.Conv2d(128, 256, kernel_size=1, stride=2)
            self.frozen = C.Conv2d(128, 128, kernel_size=1)
            self.frozen.weight.requires_grad_(False)
            self.fc = C.Conv2d(32, 64, kernel_size=7)
            self.fc.full_window = True

    net = Net()
    before = C.conv_precision()
    try:
        C.set_conv_precision("fp32")
        plan = C._build_plan(net, torch.device("cpu"))
        C.set_conv_precision("bf16")
        plan16 = C._build_plan(net, torch.device("cpu"))
    finally:
        C.set_conv_precision(before)
    assert plan.precision == "fp32" and plan16.precision == "bf16"
    assert plan.convs == [net.stem, net.c3, net.up, net.c1, net.down, net.frozen]          # full_window: skipped
    cl = torch.channels_last
    assert net.c3.weight.is_contiguous(memory_format=cl) and not net.c3.weight.is_contiguous()
    assert net.stem.weight.is_contiguous() and net.fc.weight.is_contiguous()
    assert plan.tr == [net.c3, net.up, net.c1, net.down]                # stride 1 or 1x1, 16-aligned, trainable
    assert all(w is m.weight for w, m in zip(plan.tr_weights, plan.tr)) and len(plan.tr_weights) == 4
    assert all(f.weight is f.module.weight for f in plan.frag)
    assert [tuple(t.shape) for t in plan.wts] == [(32, 3, 3, 32), (32, 1, 1, 128), (128, 1, 1, 128), (128, 1, 1, 256)]
    # the frozen layer's forward copy needs no W^T
    assert [(f.module, f.kind, f.tr_index) for f in plan.frag] == \
        [(net.c1, "fwd", -1), (net.c1, "dgrad", 2), (net.frozen, "fwd", -1)]
    assert all(f.copy.numel() == 128 * 128 for f in plan.frag)

    def tiles(m):
        co, ci = m.weight.shape[:2]
        return math.ceil(co / 32) * math.ceil(ci / 32)
    bases, base = [], 0
    for m in plan.tr:
        bases.append(base)
        base += m.weight.shape[2] * m.weight.shape[3] * tiles(m)
    for f in plan.frag:
        bases.append(base)
        base += tiles(f.module)
    assert bases == [0, 9, 13, 29, 61, 77, 93] and base == 109
    assert list(plan.desc["tile_base"]) == bases and plan.tiles == base
    assert list(plan.desc["pad"]) == [0, 0, 0, 0, 3, 1, 3]             # flags: 1 fragment-major, 2 no transpose
    assert list(plan.desc["taps"]) == [9, 1, 1, 1, 1, 1, 1]
    assert [(int(r), int(c)) for r, c in zip(plan.desc["rows"], plan.desc["cols"])] == \
        [(32, 32), (128, 32), (128, 128), (256, 128), (128, 128), (128, 128), (128, 128)]
    assert list(plan.desc["src"][:4]) == [m.weight.data_ptr() for m in plan.tr]
    assert list(plan.desc["dst"]) == [t.data_ptr() for t in plan.wts] + [f.copy.data_ptr() for f in plan.frag]
    assert plan.table is not None and plan.table.numel() == plan.desc.nbytes
    # a 16-bit plan: no fragment-major copies, a 16-bit destination per weight with Cin % 32 == 0 and per W^T
    assert plan16.frag == [] and len(plan16.desc) == 4 and plan16.tiles == 61
    assert [t.data_ptr() for t in plan16.lowp_srcs[:5]] == \
        [m.weight.data_ptr() for m in (net.c3, net.up, net.c1, net.down, net.frozen)]
    assert plan16.lowp_srcs[5:] == plan16.wts
    assert all(d.dtype == torch.bfloat16 and d.numel() == s.numel() for s, d in zip(plan16.lowp_srcs, plan16.lowp_dsts))
    assert plan.lowp_srcs == [] and plan.lowp_dsts == []
    # gradient slots: every trainable conv weight / bias, and the BatchNorm block
    assert ("dw", net.c1.weight.data_ptr()) in plan.slots and ("dw", net.frozen.weight.data_ptr()) not in plan.slots
    assert plan.slots[("dw", net.c1.weight.data_ptr())].numel == 128 * 128
    bn = plan.slots[("bn", net.bn3.weight.data_ptr())]
    assert bn.numel == 96 and bn.partner == net.c3.bias.data_ptr() and bn.owner() is net.bn3.weight
