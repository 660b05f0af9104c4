"""CPU: the host-side pieces the transformer, classify and front-end blocks share -- ops.weight_view (the persistent conv-weight view
of a Linear parameter), ops._ParamRows (rows of a parameter as a gradient owner) and ops.join_param_rows (the in-projection join).
Pure torch: no GPU, no kernel."""
import torch
import torch.nn as nn

from dedark_yolo_amd import ops


def _registered(v):
    return sum(1 for r in ops._extra_pack_views if r() is v)


def test_weight_view_is_persistent_and_follows_the_storage():
    p = nn.Parameter(torch.arange(24.0).reshape(6, 4))
    v = ops.weight_view(p, (6, 4, 1, 1))
    assert ops.weight_view(p, (6, 4, 1, 1)) is v and ops.weight_view(p, [6, 4, 1, 1]) is v
    assert v.shape == (6, 4, 1, 1) and v.data_ptr() == p.data_ptr() and not v.requires_grad
    assert _registered(v) == 1
    p.data = p.data.clone()
    v2 = ops.weight_view(p, (6, 4, 1, 1))
    assert v2 is not v and v2.data_ptr() == p.data_ptr() != v.data_ptr()
    assert ops.weight_view(p, (6, 4, 1, 1)) is v2
    assert _registered(v2) == 1 and _registered(v) == 1


def test_row_range_view_aliases_exactly_its_rows():
    p = nn.Parameter(torch.arange(48.0).reshape(12, 4))
    vs = [ops.weight_view(p, (4, 4, 1, 1), 4 * i, 4 * i + 4) for i in range(3)]
    whole = ops.weight_view(p, (12, 4, 1, 1))
    assert len({id(v) for v in vs + [whole]}) == 4 and all(_registered(v) == 1 for v in vs + [whole])
    for i, v in enumerate(vs):
        assert ops.weight_view(p, (4, 4, 1, 1), 4 * i, 4 * i + 4) is v
        assert v.data_ptr() == p.data_ptr() + 16 * i * p.element_size() and torch.equal(v.reshape(4, 4), p.detach()[4 * i:4 * i + 4])
    with torch.no_grad():
        p[4:8] = -1.0                                         # a write to the parameter shows in view 1 and in no other
    assert bool((vs[1] == -1).all()) and not bool((vs[0] == -1).any()) and not bool((vs[2] == -1).any())
    vs[2].fill_(-7.0)                                         # and a write through a view lands in its rows alone
    assert bool((p.detach()[8:] == -7).all()) and not bool((p.detach()[:8] == -7).any())


def test_views_stay_out_of_the_state_dict():
    from dedark_yolo_amd.nn import modules
    for m in (modules.TransformerLayer(32, 4), modules.TransformerEncoderLayer(32, 64, 4), modules.Classify(16, 10)):
        keys = list(m.state_dict())
        lin = [q for q in m.parameters() if q.dim() == 2]
        assert lin
        views = [ops.weight_view(q, (*q.shape, 1, 1)) for q in lin]
        if hasattr(m, "ma"):
            views += [ops.weight_view(m.ma.in_proj_weight, (32, 32, 1, 1), 32 * i, 32 * i + 32) for i in range(3)]
        assert list(m.state_dict()) == keys
        sd = m.state_dict()
        assert not any(any(v.data_ptr() == t.data_ptr() and v.shape == t.shape for t in sd.values()) for v in views)


def test_param_rows_follow_the_parameter():
    p = nn.Parameter(torch.arange(24.0).reshape(6, 4))
    r = ops._ParamRows(p, 2, 4)
    assert r.shape == (2, 4) and r.requires_grad and r._dy_direct is False and r.grad is None
    assert torch.equal(r.detach(), p.detach()[2:4]) and not r.detach().requires_grad
    p.grad = torch.zeros(6, 4)
    p._dy_direct = True
    assert r._dy_direct is True and r.grad.shape == (2, 4) and r.grad.data_ptr() == p.grad.data_ptr() + 8 * 4
    r.grad.fill_(3.0)                                         # what a kernel writes through the proxy is in p.grad
    assert bool((p.grad[2:4] == 3).all()) and float(p.grad.sum()) == 24.0
    p.requires_grad_(False)
    assert not r.requires_grad
    b = nn.Parameter(torch.arange(6.0))
    rb = ops._ParamRows(b, 4, 6)
    assert rb.shape == (2,) and torch.equal(rb.detach(), torch.tensor([4.0, 5.0]))


class _Tape:
    def __init__(self):
        self.pgrads = {}


def test_in_projection_join():
    C_ = 8
    w, b = nn.Parameter(torch.zeros(3 * C_, C_)), nn.Parameter(torch.zeros(3 * C_))
    other = nn.Parameter(torch.zeros(3))
    gw, gb = torch.randn(3 * C_, C_), torch.randn(3 * C_)
    tape = _Tape()
    tape.pgrads[other] = torch.ones(3)
    for i in (2, 0, 1):                                       # filed in backward order, joined in row order
        r0, r1 = i * C_, (i + 1) * C_
        tape.pgrads[ops._ParamRows(w, r0, r1)] = gw[r0:r1].reshape(C_, C_, 1, 1).clone()     # the conv weight gradient's shape
        tape.pgrads[ops._ParamRows(b, r0, r1)] = gb[r0:r1].clone()
    ops.join_param_rows(tape, w)
    assert torch.equal(tape.pgrads[w], gw) and b not in tape.pgrads
    ops.join_param_rows(tape, b)
    assert torch.equal(tape.pgrads[b], gb) and tape.pgrads[b].shape == (3 * C_,)
    assert set(map(id, tape.pgrads)) == {id(w), id(b), id(other)} and torch.equal(tape.pgrads[other], torch.ones(3))
    # direct placement: nothing was filed, nothing moves
    tape = _Tape()
    tape.pgrads[other] = torch.ones(3)
    before = dict(tape.pgrads)
    ops.join_param_rows(tape, w)
    ops.join_param_rows(tape, b)
    assert list(tape.pgrads) == list(before) and tape.pgrads[other] is before[other]


def test_modules_reexports_param_rows():
    from dedark_yolo_amd.nn import modules
    assert modules._ParamRows is ops._ParamRows
