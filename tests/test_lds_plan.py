"""The dynamic-LDS plan both launchers use (csrc/hip/lds_plan.h), through
C.lds_plan: how a block's LDS budget is split between the top-of-tree node
cache and the per-thread traversal stacks.  Host arithmetic only, no GPU.

With budget B = E(occ) * 256 * 8 bytes and 128-byte nodes:
  n_cached = min(request, n_nodes4, (B - 4*256*8) / 128)
  lds_max  = (B - n_cached * 128) / (256*8)
  lds_n    = lds_req if 0 <= lds_req < lds_max else lds_max
  shmem    = lds_n * 2048 + n_cached * 128
"""
import itertools

import pytest

import hippt

C = hippt.C
NODE = 128
ENTRY = 256 * 8


def entries(occ):
    """Stack entries of LDS per block at `occ` waves/SIMD."""
    return {3: 26, 4: 20, 5: 16, 6: 12}[min(max(occ, 3), 6)]


def plan(occ, in_lds, n_nodes4, cache_req, lds_req=-1, drop_cache=False):
    return C.lds_plan(occ, in_lds, drop_cache, n_nodes4, NODE, cache_req, lds_req)


@pytest.mark.parametrize("args,expect", [
    ((4, True, 10000, 64, -1), (16, 64, 40960)),
    ((4, True, 2, 64, -1), (19, 2, 39168)),
    ((4, True, 10000, 0, -1), (20, 0, 40960)),
    ((4, True, 10000, 4096, -1), (4, 256, 40960)),
    # a 256-node request beside the 12-entry budget: the cache gives way,
    # it no longer takes more than the block is allocated
    ((6, True, 10000, 256, -1), (4, 128, 24576)),
    ((6, True, 10000, 64, -1), (8, 64, 24576)),
    ((3, True, 10000, 64, -1), (22, 64, 53248)),
    ((5, True, 10000, 64, -1), (12, 64, 32768)),
    ((4, True, 400, 1, 1), (1, 1, 2176)),
    ((4, True, 400, 0, 0), (0, 0, 0)),
    ((4, True, 400, 0, 99), (20, 0, 40960)),
])
def test_exact_plans(args, expect):
    assert plan(*args) == expect


def test_scratch_stack():
    # HIPPT_WF_STACK=scratch: no LDS at all
    assert plan(4, False, 10000, 64, drop_cache=True) == (0, 0, 0)
    # HIPPT_STACK=scratch: the cache stays, sized as beside an LDS stack
    assert plan(4, False, 10000, 64, drop_cache=False) == (0, 64, 8192)
    assert plan(6, False, 10000, 256, drop_cache=False) == (0, 128, 16384)


def test_default_argument_is_no_lds_request():
    assert C.lds_plan(4, True, False, 10000, NODE, 64) == (16, 64, 40960)


def test_invariants():
    for occ, req, n_nodes4, in_lds, drop, lds_req in itertools.product(
            range(10), [0, 1, 15, 16, 17, 64, 128, 129, 192, 193, 256, 257, 5000],
            [1, 2, 100, 10000], [True, False], [True, False], [-1, 0, 1, 3, 100]):
        lds_n, n_cached, shmem = plan(occ, in_lds, n_nodes4, req, lds_req, drop)
        where = (occ, req, n_nodes4, in_lds, drop, lds_req)
        assert lds_n >= 0 and n_cached >= 0, where
        assert shmem == lds_n * ENTRY + n_cached * NODE, where
        assert shmem <= entries(occ) * ENTRY, where
        assert n_cached <= n_nodes4, where
        if in_lds and lds_req < 0:
            assert lds_n >= 4, where
        if not in_lds:
            assert lds_n == 0 and (n_cached == 0 or not drop), where
