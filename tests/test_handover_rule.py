"""cugp_pipe_block_for: tile rows handed to the inverse streams at a time, by matrix size (pure arithmetic: no device)."""
from cugp_amd import capi

NT_MAX = 160                                   # 20480 rows: beyond every size the schedule was measured at


def blocks():
    lib = capi.lib()
    return [lib.cugp_pipe_block_for(nt) for nt in range(1, NT_MAX + 1)]


def test_block_sizes_are_bounded_and_monotone():
    w = blocks()
    assert all(1 <= v <= 16 for v in w), w
    assert all(a <= b for a, b in zip(w, w[1:])), w


def test_block_sizes_at_the_measured_shapes():
    """The sizes the rule was chosen at: 4096, 6000, 8192, 10000 and 16384 rows; single tiles for the smallest matrices."""
    w = blocks()
    assert [w[nt - 1] for nt in (32, 47, 64, 79, 128)] == [2, 3, 5, 8, 8]
    assert w[:8] == [1] * 8 and w[8] == 2
