"""An autouse fixture for GPU test modules that should leave torch's caching allocator as they found it.

Why: the suite runs in ONE process, and some state of the library outlives a test keyed on DEVICE ADDRESSES — the adaptive
segmented backward remembers its verdict per view under the address of the view matrix (csrc/gspl_composite.h, ADAPTIVE), and
tests/test_segmented_backward.py::test_the_adaptive_switch_asks_for_a_tail_not_for_length relies on which block the allocator hands
to its next view matrix.  Every tensor a test allocates and frees reshapes the allocator's free lists for all tests behind it.  A
module that imports this fixture allocates from a memory pool of its own, released after each test, so the default pool sees nothing
of it (except what an autograd backward allocates on the engine's thread: transient, freed before the test ends).

    from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)
"""
import pytest
import torch


@pytest.fixture(autouse=True)
def private_memory_pool(request):
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
    del pool
