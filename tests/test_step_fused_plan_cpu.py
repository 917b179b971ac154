"""Host side of the fused cast + column-sum pass (vaw_cast_colsum_plan): what it launches, what it reads and writes, and that it
refuses -- launching nothing -- whatever the summation tree of vaw_colsum would treat differently."""
from vaw_amd import ops
from vaw_amd import _lib as L

A = 1 << 20          # an aligned stand-in address


def test_plan_covers_every_column_once_and_counts_its_bytes():
    for M, N in ((1, 4), (3, 1536), (8, 56832), (256, 56832), (512, 260)):
        p = ops.cast_colsum_plan(M, N, N, N, A, 2 * A, 3 * A)
        assert p is not None and p.block == 256
        assert (p.grid_x - 1) * 256 < N <= p.grid_x * 256          # one workgroup per 256 columns, none empty
        assert p.rows_per_lane * 4 >= M > (p.rows_per_lane - 1) * 4  # four row groups, rows ascending inside each
        assert p.bytes_read == 4 * M * N and p.bytes_written == 2 * M * N + 4 * N
    wide = ops.cast_colsum_plan(256, 768, 56832, 56832, A + 4 * 768, 2 * A + 2 * 768, 3 * A + 4 * 768)      # a column window
    assert wide is not None and wide.grid_x == 3


def test_plan_refuses_what_the_column_sum_tree_treats_differently():
    ok = dict(M=8, N=64, ld_src=64, ld_dst=64, src_addr=A, dst_addr=2 * A, colsum_addr=3 * A)
    assert ops.cast_colsum_plan(**ok) is not None
    for bad in (dict(M=513), dict(M=0), dict(N=62), dict(N=0), dict(ld_src=66), dict(ld_dst=66), dict(ld_src=32), dict(src_addr=A + 4),
                dict(dst_addr=2 * A + 8), dict(src_addr=0), dict(dst_addr=0), dict(colsum_addr=0)):
        assert ops.cast_colsum_plan(**dict(ok, **bad)) is None, bad
        assert b"cast_colsum" in L.lib().vaw_last_error_string()
    # the entry point goes through the same plan before it touches the device: refused operands return an error, nothing is launched
    rc = L.lib().vaw_cast_colsum_bf16(A, 64, 2 * A, 64, 600, 64, 3 * A, 0.0, None)
    assert rc != 0 and b"512" in L.lib().vaw_last_error_string()
