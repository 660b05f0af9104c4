"""The packed operand images that ops keeps on a parameter (ops._packed_image, behind the PConv and the CRU weight packs): one image
per (transposed, dtype), handed out again without a launch while the weights stand, re-packed into the same storage after an
in-place update or ops.bump_weights_epoch(), bit for bit what a fresh pack of the new weights gives."""
import pytest
import torch

from util import rnd

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _pconv(seed=31, c3=16):
    from dedark_yolo_amd import _C, ops
    w = torch.nn.Parameter((rnd(seed, c3, c3, 3, 3, lo=-1, hi=1) / 12.0).cuda())

    def image(tr):
        return ops._pconv_packed(w, ops._w32(w), tr, BF16)

    def fresh(tr):
        out = torch.empty(9 * ((c3 + 31) // 32) * ((c3 + 15) // 16) * 512, dtype=BF16, device="cuda")
        _C.call("dy_pconv_pack", ops.ptr(ops._w32(w)), ops.ptr(out), c3, tr, ops.dt_id(BF16), ops.stream())
        return out

    return [w], image, fresh


def _cru(seed=41, G=2, N=8, C3=4, C1=8):
    from dedark_yolo_amd import _C, ops
    w3 = torch.nn.Parameter((rnd(seed, G * N, C3, 3, 3, lo=-1, hi=1) / 8.0).cuda())
    w1 = torch.nn.Parameter((rnd(seed + 1, G * N, C1, 1, 1, lo=-1, hi=1) / 8.0).cuda())

    def image(tr):
        return ops._cru_packed(w3, w1, G, tr, BF16)

    def fresh(tr):
        out = torch.empty(G * N * (9 * C3 + C1), dtype=BF16, device="cuda")
        _C.call("dy_cru_conv_pack", ops.ptr(ops._w32(w3)), ops.ptr(ops._w32(w1)), ops.ptr(out), G, N, C3, C1, tr, ops.dt_id(BF16), ops.stream())
        return out

    return [w3, w1], image, fresh


@pytest.mark.parametrize("make", [_pconv, _cru], ids=["pconv", "cru"])
def test_packed_image_is_kept_and_repacked_in_place(make, monkeypatch):
    from dedark_yolo_amd import ops
    params, image, fresh = make()
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    first = {tr: image(tr) for tr in (0, 1)}
    assert len(calls) == 2 and first[0] is not first[1]
    for tr in (0, 1):
        assert torch.equal(first[tr], fresh(tr))
    assert not torch.equal(first[0], first[1])

    def handed_out_again():
        n = len(calls)
        for tr in (0, 1):
            assert image(tr) is first[tr]
        assert len(calls) == n, calls[n:]                   # no entry of the library was called: nothing launched

    def repacked():
        n = len(calls)
        for tr in (0, 1):
            ptr = first[tr].data_ptr()
            got = image(tr)
            assert got is first[tr] and got.data_ptr() == ptr       # the same storage
            assert torch.equal(got, fresh(tr))
        assert len(calls) == n + 2, calls[n:]
        handed_out_again()

    handed_out_again()
    for p in params:                                        # an in-place update of either weight (it bumps the version counter)
        before = [first[tr].clone() for tr in (0, 1)]
        with torch.no_grad():
            p.mul_(-1.5)
        repacked()
        assert not torch.equal(first[0], before[0]) and not torch.equal(first[1], before[1])
    before = [first[tr].clone() for tr in (0, 1)]
    params[-1].data.add_(0.25)                              # a write past the version counter, as the fused optimizer's, ...
    handed_out_again()
    ops.bump_weights_epoch()                                # ... which announces itself this way
    repacked()
    assert not torch.equal(first[0], before[0]) and not torch.equal(first[1], before[1])
