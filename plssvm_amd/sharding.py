"""Row-block sharding of the implicit matrix across the GPUs of one node -- host-side plumbing.

The reference splits the FEATURE dimension across devices, for the linear kernel only, and sums the partial results
through the host (include/plssvm/backends/gpu_csvm.hpp:283-299, :449-475).  Here every rank (one process per GPU) owns a
contiguous run of 128-row blocks of the implicit matrix for all three kernels; the data matrix is replicated.  Default
(symmetric variant: only the tiles on/below the diagonal are evaluated): blocks dealt by equal AREA, one RCCL all-reduce of
the partial K*d vectors per implicit matvec.  Full-square variant: equal runs of blocks, one all-gather of the K*d slices.
This module holds the partition arithmetic (identical to ``shard_blocks`` in plssvm_amd/csrc/lssvm_geometry.cpp),
the flop accounting bench.py uses, and the bootstrap of the library's RCCL communicator over an existing
``torch.distributed`` process group.
"""

from __future__ import annotations

TILE = 128  # rows per block of the tile kernel (plssvm_amd/csrc/lssvm_geometry.hpp)

__all__ = ["TILE", "row_block_partition", "sym_block_partition", "work_share", "triangle_share", "padded_vector_length", "exchange_unique_id", "init_library_communicator", "connect_peers"]


def row_block_partition(n: int, world: int):
    """Return ``[(row_begin, row_end), ...]`` per rank for a reduced system of size ``n`` (= num_points - 1).

    Blocks of 128 rows are dealt in equal contiguous runs; trailing ranks may own fewer (or no) rows.  Every evaluated
    row costs the same (full square, no symmetry), so equal rows == equal work."""
    if n < 1 or world < 1:
        raise ValueError("n and world must be positive")
    tiles = (n + TILE - 1) // TILE
    per_rank = (tiles + world - 1) // world
    out = []
    for r in range(world):
        b0 = min(r * per_rank, tiles)
        b1 = min(b0 + per_rank, tiles)
        out.append((min(b0 * TILE, n), min(b1 * TILE, n)))
    return out


def sym_block_partition(n: int, world: int, weights=None):
    """Symmetric variant (only the tiles on/below the diagonal are evaluated): row block ``ib`` costs ``ib + 1`` tiles, so the
    blocks are dealt by equal AREA -- boundary of rank r = tiles * sqrt(r / world) rounded to an EVEN block index (the 256-row
    workgroups of the tile kernel work on block pairs; ``sym_block_boundary`` in plssvm_amd/csrc/lssvm_geometry.cpp).  ``weights``
    (one positive number per rank; ``lssvm_mi355_set_shard_weights``): rank r gets ``weights[r] / sum`` of the area instead of ``1 / world``
    -- devices of unequal pace.  Returns ``[(block_begin, block_end), ...]``."""
    import math

    def llround(x: float) -> int:  # C's llround for x >= 0 (half away from zero; x - floor(x) is exact, x + 0.5 need not be: ADVICE r04)
        f = math.floor(x)
        return int(f) + (1 if x - f >= 0.5 else 0)

    tiles = (n + TILE - 1) // TILE
    if weights is not None and len(weights) == world:
        total = 0.0
        for w in weights:  # (running sums in the library's order: the two partitions must agree to the bit)
            total += float(w)
        shares, before = [], 0.0
        for r in range(1, world):
            before += float(weights[r - 1])
            shares.append(before / total)
    else:
        shares = [r / world for r in range(1, world)]
    bounds = [0] + [min(max(2 * llround(0.5 * tiles * math.sqrt(sh)), 0), tiles) for sh in shares] + [tiles]
    return [(bounds[r], max(bounds[r], bounds[r + 1])) for r in range(world)]


def work_share(n: int, world: int, rank: int, symmetric: bool, weights=None):
    """(algorithmic, executed) multiply-add counts per feature of one implicit matvec launch on ``rank``.

    Algorithmic = this rank's share of the full n x n square (no symmetry credit in the metric);
    executed = the tile elements it really evaluates (half of it, plus the diagonal, in the symmetric variant)."""
    if not symmetric:
        r0, r1 = row_block_partition(n, world)[rank]
        return float(r1 - r0) * n, float(r1 - r0) * n
    tiles = (n + TILE - 1) // TILE
    b0, b1 = sym_block_partition(n, world, weights)[rank]
    evaluated_tiles = (b1 * (b1 + 1) - b0 * (b0 + 1)) // 2          # sum of (ib + 1)
    mirrored_tiles = (b1 * (b1 - 1) - b0 * (b0 - 1)) // 2           # strictly lower tiles count twice in the square
    full_tiles = float(tiles) * tiles
    algorithmic = (evaluated_tiles + mirrored_tiles) / full_tiles * float(n) * n
    executed = evaluated_tiles * float(TILE) * TILE
    return algorithmic, executed


def triangle_share(n: int, world: int, rank: int, weights=None) -> float:
    """Multiply-adds per feature of the reference's own algorithm (kernel entries with j <= i only,
    src/plssvm/backends/OpenMP/svm_kernel.cpp:36-39) that fall into ``rank``'s row blocks of the symmetric partition."""
    b0, b1 = sym_block_partition(n, world, weights)[rank]
    r0, r1 = min(b0 * TILE, n), min(b1 * TILE, n)
    return (r1 * (r1 + 1) - r0 * (r0 + 1)) / 2.0


def padded_vector_length(n: int, world: int) -> int:
    """Length of the device vectors: every rank's all-gather slice has the same size ``per_rank * 128``."""
    tiles = (n + TILE - 1) // TILE
    per_rank = (tiles + world - 1) // world
    return per_rank * world * TILE


def exchange_unique_id(dist, get_unique_id, device=None) -> bytes:
    """Rank 0 draws the 128-byte RCCL unique id, every rank receives it through ``dist.broadcast``.

    ``dist`` is an initialised ``torch.distributed``; ``device`` is the tensor device for the broadcast ("cuda" for the
    nccl backend, None/"cpu" for gloo)."""
    import torch

    uid = torch.zeros(128, dtype=torch.uint8)
    if dist.get_rank() == 0:
        uid = torch.frombuffer(bytearray(get_unique_id()), dtype=torch.uint8).clone()
    if device is not None:
        uid = uid.to(device)
    dist.broadcast(uid, src=0)
    return bytes(uid.cpu().numpy().tobytes())


def init_library_communicator(dist, local_device: int, device="cuda") -> None:
    """Create libplssvm_amd's own RCCL communicator for this process from a torch.distributed process group (``device`` = where the
    id travels: "cuda" for the nccl backend, None for gloo)."""
    from . import backend

    uid = exchange_unique_id(dist, backend.comm_get_unique_id, device=device)
    backend.comm_init(local_device, dist.get_rank(), dist.get_world_size(), uid)


def connect_peers(dist, problem) -> None:
    """One process per GPU over HIP IPC (no RCCL inside the library): every rank exports its blob, all ranks receive all blobs in rank
    order through ``dist.all_gather_object`` (any backend) and connect (``lssvm_mi355_problem_ipc_export`` / ``_connect``)."""
    blobs = [None] * dist.get_world_size()
    dist.all_gather_object(blobs, problem.ipc_export())
    problem.ipc_connect(blobs)
    dist.barrier()  # every rank has mapped every vector before anyone starts to exchange
