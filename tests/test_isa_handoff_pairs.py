"""CPU test (hipcc cross-compiles gfx950 without a GPU): pg_round_pairs_kernel, GICP_HIP's round kernel for pairs that each name their own
target, hands its partial rows to the pair's closing workgroup by the same instruction sequence as pg_round_kernel
(tests/test_isa_handoff.py: write-through row store, drain, barrier, agent-scope ticket, barrier, coherent row loads), and pays no
cache-wide write-back / invalidate for it."""
import os
import re
import subprocess

import pytest

from test_isa_handoff import CSRC, _body, _first

PREFIX = "_ZN3dgs21pg_round_pairs_kernelE"


@pytest.fixture(scope="module")
def listing():
    subprocess.check_call(["make", "-C", CSRC, "isa", "-j2"], stdout=subprocess.DEVNULL)
    return open(os.path.join(CSRC, "build", "pcl_gicp.s")).read()


def test_the_pairs_kernel_hands_its_rows_over_in_the_documented_order(listing):
    ln = _body(listing, PREFIX)
    store = _first(ln, r"^global_store_dwordx2 .* sc1\b")
    assert store >= 0, "row store is not write-through (sc1)"
    barrier1 = _first(ln, r"^s_barrier", store)
    drain = _first(ln, r"^s_waitcnt vmcnt\(0\)$", store)
    assert 0 <= drain < barrier1, "the storing wave does not drain its stores before the barrier"
    ticket = _first(ln, r"^global_atomic_add \S+, \S+, \S+, .* sc0\b", barrier1)
    assert ticket > barrier1, "the ticket is not taken behind the barrier"
    assert _first(ln, r"^global_atomic_add", store) == ticket, "another atomic sits between the row store and the ticket"
    barrier2 = _first(ln, r"^s_barrier", ticket)
    load = _first(ln, r"^global_load_dwordx2 .* sc1\b", ticket)
    assert barrier2 > ticket and load > barrier2, "the closing workgroup's row loads are not coherent (sc1) loads behind the second barrier"
    reset = _first(ln, r"^global_store_dword \S+, \S+, .* sc1\b", ticket)
    assert ticket < reset < barrier2, "the ticket is not reset by its taker with an agent-scope store"
    assert not any(re.match(r"buffer_wbl2|buffer_inv", x) for x in ln), "a cache-wide write-back / invalidate crept into the kernel"
