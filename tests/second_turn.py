"""Deep matrices by repetition, for the cases in which a workgroup of a capped grid takes a second turn (tests/test_gpu_rescue.py,
test_gpu_nearest.py, test_gpu_recombinant.py): the hap-walk launch has at most 4096 one-wave workgroups, each walking the runs of 64
reads x, x + 4096, ..., so a second run is taken only above 4096 * 64 = 262 144 reads.  Every answer of those stages depends on a
read's own row and the table only, so for rows that are a block repeated with a tail — read i is block[i mod len(block)] — the
per-read outputs are the block's, tiled, and every count is the block's times the repeats plus the tail's
(tests/test_second_turn_host.py checks that against the mirrors run in full).  The mirrors then never run over 262k reads, and
the planes are the block's planes repeated bytewise on the device.  numpy only, torch where a tensor is made."""
import numpy as np

from minorseq_amd import msa

GRID_CAP, RUN = 4096, 64
ONE_TURN = GRID_CAP * RUN                                  # 262 144 reads: 4096 runs, one turn each
# reads of a block: a multiple of 8, so its planes repeat bytewise, that does not divide 262 144 — read 262 144 + i then holds another
# row than read i, which the same lane of the same workgroup walked in its first turn (262 144 mod 2040 = 1024: the row 1024 further on)
BLOCK = 2040
# (reads, what the count is): the control; one read in a 4097th run, workgroup 0's second; workgroups 0 .. 63 in a second turn that
# workgroup 64 does not take, the last of them with one read
COUNTS = [(ONE_TURN, "4096 runs"), (ONE_TURN + 1, "4097 runs"), (ONE_TURN + RUN * 63 + 1, "4160 runs")]
assert [-(-n // RUN) for n, _ in COUNTS] == [4096, 4097, 4160] and BLOCK % 8 == 0 and ONE_TURN % BLOCK == 1024 and BLOCK % RUN != 0


def split(n, block=BLOCK):
    """(whole repeats, reads of the tail)."""
    return n // block, n % block


def tiled_rows(block_rows, n):
    reps, tail = split(n, len(block_rows))
    return np.concatenate([np.tile(block_rows, (reps, 1)), block_rows[:tail]])


def tiled(per_read, n):
    """A per-read output of the block as the output of the n tiled reads."""
    reps, tail = split(n, len(per_read))
    return np.concatenate([np.tile(per_read, reps), per_read[:tail]])


def summed(block_count, tail_count, n, block):
    reps, _ = split(n, block)
    return (reps * block_count.astype(np.uint64) + tail_count.astype(np.uint64)).astype(block_count.dtype)


def second_turn_reads(n):
    """The reads of the runs that are some workgroup's second."""
    return slice(ONE_TURN, n)


def adopt_tiled(j, block_rows, n):
    """The planes of tiled_rows(block_rows, n) as a torch tensor that `j` adopts: the block packed once and repeated bytewise, the
    tail packed with its own padding (code 6).  Returns the tensor."""
    import torch
    assert len(block_rows) % 8 == 0
    reps, tail = split(n, len(block_rows))
    head = reps * (len(block_rows) // 8)
    tail_bytes = max((tail + 7) // 8, 8 * -(-n // RUN) - head, 0)
    tail_bytes += -(head + tail_bytes) % 16                # the whole stride a multiple of 16; what the tail does not fill is code 6
    parts = [torch.from_numpy(msa.pack_planes(block_rows, len(block_rows) // 8)).cuda().repeat(1, 1, reps)]
    if tail_bytes:
        parts.append(torch.from_numpy(msa.pack_planes(block_rows[:tail], tail_bytes)).cuda())
    t = torch.cat(parts, dim=2).contiguous()
    torch.cuda.synchronize()
    stride = t.shape[2]
    assert stride % 16 == 0 and stride >= (n + 7) // 8 and stride >= 8 * -(-n // RUN)
    j.adopt(t.data_ptr(), n, block_rows.shape[1], stride, keep_alive=t)
    return t
