"""csrc/dy_plan.h on the host: the weight-gradient split plan against the arithmetic the PConv and CRU launchers used to write out by
hand, the overlap test of two NHWC views against a byte-set intersection, the access width against its definition.  No GPU: the
header needs no HIP, so a small shim is compiled with the host compiler into tmp_path and loaded with ctypes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dedark_yolo_amd", "csrc")

SHIM = r"""
#include <vector>
#include "dy_plan.h"
extern "C" {
void sh_plan(const long* M, const long* want, const long* fit, long n, long min_pixels, long step, long* splits, long* chunk) {
  for (long i = 0; i < n; ++i) {
    const dy_route::WgradSplits p = dy_route::plan_wgrad_splits(M[i], want[i], min_pixels, step, fit[i], dy_route::kNoGridCap);
    splits[i] = p.splits;
    chunk[i] = p.chunk;
  }
}
int sh_view_bytes(unsigned long p, long ld, int C, int es) { return dy_view_bytes((const void*)p, ld, C, es); }
int sh_overlap(unsigned long s, long s_ld, long sp, int sC, unsigned long d, long d_ld, long dp, int dC, int es) {
  return dy_views_overlap((const void*)s, s_ld, sp, sC, (const void*)d, d_ld, dp, dC, es) ? 1 : 0;
}
// the definition: the bytes of the lanes [0, sC) of sp pixels and of the lanes [0, dC) of dp pixels, as sets
static bool share_a_byte(long s, long s_ld, long sp, int sC, long d, long d_ld, long dp, int dC, int es) {
  const long lo = s < d ? s : d;
  const long s_end = s + ((sp - 1) * s_ld + sC) * es, d_end = d + ((dp - 1) * d_ld + dC) * es;
  std::vector<char> used((s_end > d_end ? s_end : d_end) - lo, 0);
  for (long p = 0; p < sp; ++p)
    for (long b = 0; b < (long)sC * es; ++b) used[s + p * s_ld * es + b - lo] = 1;
  for (long p = 0; p < dp; ++p)
    for (long b = 0; b < (long)dC * es; ++b)
      if (used[d + p * d_ld * es + b - lo]) return true;
  return false;
}
// every byte offset of the destination within two source rows either way; counts[0] cases, [1] answers that differ from the
// definition, [2] of those the ones that say "disjoint" where bytes are shared
void sh_overlap_sweep(long s_ld, long sp, int sC, long d_ld, long dp, int dC, int es, long* counts) {
  const long base = 1L << 20, row = s_ld * es;
  for (long off = -2 * row; off <= 2 * row; ++off) {
    const bool want = share_a_byte(base, s_ld, sp, sC, base + off, d_ld, dp, dC, es);
    const bool got = dy_views_overlap((const void*)base, s_ld, sp, sC, (const void*)(base + off), d_ld, dp, dC, es);
    counts[0] += 1;
    counts[1] += got != want;
    counts[2] += want && !got;
  }
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("launch_plan")
    src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "liblaunch_plan_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    lib = C.CDLL(so)
    lib.sh_view_bytes.argtypes = [C.c_ulong, C.c_long, C.c_int, C.c_int]
    lib.sh_overlap.argtypes = [C.c_ulong, C.c_long, C.c_long, C.c_int, C.c_ulong, C.c_long, C.c_long, C.c_int, C.c_int]
    lib.sh_overlap_sweep.argtypes = [C.c_long, C.c_long, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p]
    lib.sh_plan.argtypes = [C.c_void_p] * 3 + [C.c_long] * 3 + [C.c_void_p] * 2
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _plan(shim, M, want, fit, min_pixels, step):
    M, want, fit = (np.ascontiguousarray(a, dtype=np.int64) for a in (M, want, fit))
    splits, chunk = np.empty_like(M), np.empty_like(M)
    shim.sh_plan(_p(M), _p(want), _p(fit), len(M), min_pixels, step, _p(splits), _p(chunk))
    return splits, chunk


N_PLANS = 400_000


def _plan_inputs(seed):
    """M in [1, 3e6] (a quarter of them small, where the clamps to M bind), fit and tile counts in [1, 2000]"""
    rng = np.random.default_rng(seed)
    M = rng.integers(1, 3_000_001, N_PLANS)
    M[::4] = rng.integers(1, 5000, len(M[::4]))
    return M, rng.integers(1, 2001, N_PLANS), rng.integers(1, 2001, N_PLANS)


def test_plan_equals_the_pconv_chunks(shim):
    """pconv.hip's launch_wgrad as it stood: at least 2048 pixels per chunk, at most 512 chunks and what the scratch holds"""
    M, fit, _ = _plan_inputs(1)
    n = np.minimum(np.minimum((M + 2047) // 2048, 512), fit)
    chunk = (M + n - 1) // n
    n = (M + chunk - 1) // chunk
    splits, got_chunk = _plan(shim, M, np.full_like(M, 512), fit, 2048, 1)
    assert np.array_equal(splits, n) and np.array_equal(got_chunk, chunk)


def test_plan_equals_the_cru_ranges(shim):
    """dy_cru_conv_wgrad as it stood: whole steps of 32 pixels, about 1024 blocks over the tiles, as many as the scratch holds"""
    M, fit, tiles = _plan_inputs(2)
    steps = (M + 31) // 32
    s = np.maximum(np.minimum(np.minimum(1024 // tiles, fit), steps), 1)
    rng_ = (steps + s - 1) // s * 32
    s = (M + rng_ - 1) // rng_
    splits, chunk = _plan(shim, M, 1024 // tiles, fit, 32, 32)
    assert np.array_equal(splits, s) and np.array_equal(chunk, rng_)


def _configs(seed, n, equal_ld):
    """(s_ld, sp, sC, d_ld, dp, dC, es): pixel strides <= 24, channel counts <= 12, up to 6 pixels, 2- and 4-byte elements"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        sC, dC = (int(v) for v in rng.integers(1, 13, 2))
        s_ld, d_ld = int(rng.integers(sC, 25)), int(rng.integers(dC, 25))
        if equal_ld:
            s_ld = d_ld = max(s_ld, d_ld)
        elif s_ld == d_ld:
            continue
        out.append((s_ld, int(rng.integers(1, 7)), sC, d_ld, int(rng.integers(1, 7)), dC, int(rng.choice([2, 4]))))
    return out


def _sweep(shim, configs):
    counts = np.zeros(3, dtype=np.int64)
    for s_ld, sp, sC, d_ld, dp, dC, es in configs:
        shim.sh_overlap_sweep(s_ld, sp, sC, d_ld, dp, dC, es, _p(counts))
    return counts


def test_overlap_is_exact_inside_one_buffer(shim):
    """equal pixel strides: the answer is the byte-set intersection, at every byte offset within two rows"""
    # the corners first: one pixel, full rows, the widest and the narrowest lanes
    corners = [(ld, sp, sC, ld, dp, dC, es) for ld in (12, 13, 24) for sp in (1, 6) for dp in (1, 6) for sC in (1, 12) for dC in (1, 12)
               for es in (2, 4)]
    cases, wrong, _ = _sweep(shim, corners + _configs(3, 3000, True))
    print(f"{cases} cases, {wrong} wrong")
    assert cases > 500_000 and wrong == 0


def test_overlap_never_misses_between_buffers(shim):
    """unequal pixel strides: intersecting extents are refused outright, so shared bytes are never called disjoint"""
    cases, wrong, missed = _sweep(shim, _configs(4, 3000, False))
    print(f"{cases} cases, {wrong} refused without a shared byte, {missed} missed")
    assert cases > 500_000 and missed == 0


def _overlap_one_count(s, s_ld, sp, d, d_ld, dp, Cn, es):
    """dwconv.hip's views_overlap as it stood, one channel count for both views"""
    cb = Cn * es
    s1, d1 = s + (sp - 1) * s_ld * es + cb, d + (dp - 1) * d_ld * es + cb
    if s1 <= d or d1 <= s:
        return False
    if s_ld != d_ld:
        return True
    row = s_ld * es
    off = (d - s) % row
    return off < cb or row - off < cb


def test_overlap_agrees_with_the_depthwise_cases(shim):
    """test_dwconv_rejects_bad_arguments: the halves [0, 8), [4, 12) and [8, 16) of a 1x8x8x16 f32 buffer, both directions"""
    base, want = 1 << 20, {0: True, 4: True, 8: False}
    for lane, overlaps in want.items():
        for s, d in ((base, base + 4 * lane), (base + 4 * lane, base)):
            got = bool(shim.sh_overlap(s, 16, 64, 8, d, 16, 64, 8, 4))
            assert got == overlaps == _overlap_one_count(s, 16, 64, d, 16, 64, 8, 4), (lane, s, d)
    # and on a sweep of equal channel counts, stride-2 pixel counts included
    rng = np.random.default_rng(5)
    for _ in range(20000):
        Cn, es = int(rng.integers(1, 13)), int(rng.choice([2, 4]))
        s_ld = int(rng.integers(Cn, 25))
        d_ld = s_ld if rng.random() < 0.8 else int(rng.integers(Cn, 25))
        sp, dp = (int(v) for v in rng.integers(1, 65, 2))
        s = base
        d = base + int(rng.integers(-3 * s_ld, 3 * s_ld + 1)) * es
        assert bool(shim.sh_overlap(s, s_ld, sp, Cn, d, d_ld, dp, Cn, es)) == _overlap_one_count(s, s_ld, sp, d, d_ld, dp, Cn, es)


def test_view_bytes_is_its_definition(shim):
    """the widest of 16 and 8 bytes that divides the address, the bytes of a row and the bytes of the lanes; 0 = element accesses"""
    n = 0
    for es in (2, 4):
        for a in range(0, 64, es):
            for ld in range(1, 41):
                for Cn in range(1, ld + 1):
                    want = next((w for w in (16, 8) if a % w == 0 and (ld * es) % w == 0 and (Cn * es) % w == 0), 0)
                    assert shim.sh_view_bytes((1 << 20) + a, ld, Cn, es) == want, (es, a, ld, Cn)
                    n += 1
    assert n > 30000
