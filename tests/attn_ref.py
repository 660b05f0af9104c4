"""float64 numpy statement of the fused attention kernels (csrc/attn.hip: dy_attn_fwd / dy_attn_bwd): the yardstick of
tests/test_gpu_attn.py, itself checked against torch.nn.functional.multi_head_attention_forward in tests/test_c3tr_cpu.py.

Tokens are rows: q, k, v, o, do are [B, L, C] with C = H * D, head h = channels [h D, (h + 1) D).
"""
import numpy as np


def _heads(x, H):
    B, L, C = x.shape
    return np.asarray(x, dtype=np.float64).reshape(B, L, H, C // H).transpose(0, 2, 1, 3)        # [B, H, L, D]


def _tokens(x):
    B, H, L, D = x.shape
    return x.transpose(0, 2, 1, 3).reshape(B, L, H * D)


def forward(q, k, v, H, scale=None):
    """O [B, L, C], LSE [B, H, L] (log sum_j exp(scale * q_i . k_j)), P [B, H, L, L]"""
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    scale = qh.shape[-1] ** -0.5 if scale is None else scale
    s = scale * (qh @ kh.transpose(0, 1, 3, 2))
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    p = e / l
    return _tokens(p @ vh), (m + np.log(l))[..., 0], p


def backward(q, k, v, o, do, lse, H, scale=None):
    """dq, dk, dv [B, L, C] in the flash form, from the inputs the kernel gets: P = exp(scale S - lse), delta_i = sum_c dO_ic O_ic,
    dV = P^T dO, dS = P o (dO V^T - delta), dQ = scale dS K, dK = scale dS^T Q.  Also returns the dict of intermediates."""
    qh, kh, vh, oh, doh = (_heads(t, H) for t in (q, k, v, o, do))
    scale = qh.shape[-1] ** -0.5 if scale is None else scale
    p = np.exp(scale * (qh @ kh.transpose(0, 1, 3, 2)) - np.asarray(lse, dtype=np.float64)[..., None])
    dp = doh @ vh.transpose(0, 1, 3, 2)
    delta = (doh * oh).sum(-1, keepdims=True)
    ds = p * (dp - delta)
    dv = p.transpose(0, 1, 3, 2) @ doh
    dq = scale * (ds @ kh)
    dk = scale * (ds.transpose(0, 1, 3, 2) @ qh)
    return _tokens(dq), _tokens(dk), _tokens(dv), dict(p=p, dp=dp, delta=delta, ds=ds)


def forward_terms(p, v, H):
    """sum_j P_ij |V_jc|: the sum of the magnitudes of the terms that form O_ic"""
    return _tokens(p @ np.abs(_heads(v, H)))


def backward_terms(q, k, v, o, do, lse, H, scale=None):
    """The same for dq, dk, dv, with the nested sums written out: dS_ij = P_ij (sum_c dO_ic V_jc - sum_c dO_ic O_ic) has the terms
    P_ij (sum_c |dO_ic| |V_jc| + sum_c |dO_ic| |O_ic|) =: A_ij, so dQ_ic has scale sum_j A_ij |K_jc|, dK_jc has scale sum_i A_ij |Q_ic| and
    dV_jc has sum_i P_ij |dO_ic|."""
    qh, kh, vh, oh, doh = (_heads(t, H) for t in (q, k, v, o, do))
    scale = qh.shape[-1] ** -0.5 if scale is None else scale
    p = np.exp(scale * (qh @ kh.transpose(0, 1, 3, 2)) - np.asarray(lse, dtype=np.float64)[..., None])
    a = p * (np.abs(doh) @ np.abs(vh).transpose(0, 1, 3, 2) + (np.abs(doh) * np.abs(oh)).sum(-1, keepdims=True))
    tq = scale * (a @ np.abs(kh))
    tk = scale * (a.transpose(0, 1, 3, 2) @ np.abs(qh))
    tv = p.transpose(0, 1, 3, 2) @ np.abs(doh)
    return _tokens(tq), _tokens(tk), _tokens(tv)
