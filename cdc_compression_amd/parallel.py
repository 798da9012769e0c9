"""Batch sharding of the decode over the GPUs of one node.

Every image is an independent DDIM chain (no cross-image operation anywhere on the path), so the batch
is split into contiguous shards, one process + one libcdc_hip handle per GPU, weights replicated.  There
is NO collective on the data path; the only exchange is the final gather of the decoded images
(`torch.distributed.all_gather`: RCCL over xGMI with the "nccl" backend, gloo on CPU in the tests).
"""


def shard_bounds(batch, world_size, rank):
    """Contiguous, balanced [lo, hi) of `batch` images for `rank` (first `batch % world` ranks get +1)."""
    if not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} outside world of {world_size}")
    base, extra = divmod(batch, world_size)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def expand_seeds(seed, batch):
    """The per-image 64-bit seeds of a seeded decode (`seed=` of decompress / compress; include/cdc_hip.h: cdc_decode_seeded):
    an int s gives image b the seed (s + b) mod 2^64; a sequence of `batch` ints is taken as it is.  Every value must lie in
    [0, 2^64); anything else is a ValueError."""
    if isinstance(seed, bool) or (not hasattr(seed, "__index__") and not hasattr(seed, "__len__")):
        raise ValueError(f"seed must be an int or a sequence of {batch} ints, not {type(seed).__name__}")
    if hasattr(seed, "__index__") and not hasattr(seed, "__len__"):
        s = int(seed)
        if not 0 <= s < 2 ** 64:
            raise ValueError(f"seed {s} outside [0, 2^64)")
        return [(s + b) % 2 ** 64 for b in range(batch)]
    seeds = list(seed)
    if len(seeds) != batch:
        raise ValueError(f"{len(seeds)} seeds for a batch of {batch}")
    out = []
    for v in seeds:
        if isinstance(v, bool) or not hasattr(v, "__index__"):
            raise ValueError(f"seed {v!r} is not an int")
        v = int(v)
        if not 0 <= v < 2 ** 64:
            raise ValueError(f"seed {v} outside [0, 2^64)")
        out.append(v)
    return out


def sample_seeds(seed, batch, samples):
    """The seeds of `samples` seeded decodes per image (`samples=` of decompress, compress_best_of; include/cdc_hip.h states the rule):
    [batch][samples] ints.  With s_b = expand_seeds(seed, batch)[b], sample k of image b has the seed (s_b + k * 2^32) mod 2^64: sample 0
    is the seeded decode of the same `seed`, and an int seed never gives two rows the same key (images differ by +1, samples by
    +2^32).  A 2-D [batch][samples] array of ints in [0, 2^64) is taken as it is."""
    if isinstance(samples, bool) or not hasattr(samples, "__index__") or int(samples) < 1:
        raise ValueError(f"samples must be an int >= 1, not {samples!r}")
    K = int(samples)
    rows = list(seed) if hasattr(seed, "__len__") else None
    if rows and all(hasattr(r, "__len__") for r in rows):
        if len(rows) != batch:
            raise ValueError(f"{len(rows)} rows of seeds for a batch of {batch}")
        return [expand_seeds(r, K) for r in rows]
    return [[(s + (k << 32)) % 2 ** 64 for k in range(K)] for s in expand_seeds(seed, batch)]


def shard_seeds(seed, batch, world_size, rank):
    """The seeds of this rank's shard_bounds slice of a `batch`-image job: a sharded seeded decode then equals the unsharded one
    image for image (an image's draws depend on its own seed only)."""
    lo, hi = shard_bounds(batch, world_size, rank)
    return expand_seeds(seed, batch)[lo:hi]


def sharded_decode(decode_fn, init, context, world_size=1, rank=0, dist=None, global_batch=None):
    """Run `decode_fn(init_shard, context_shard) -> reconstruction shard` on this rank's slice of the
    batch and gather the full batch on every rank.

    init: [B, C, H, W] tensor or None; context: list of [B, C_l, H_l, W_l] tensors.  With
    world_size == 1 (or dist None) this is a plain call.  Shards may be ragged (B % world != 0):
    they are padded to the largest shard for the fixed-size all_gather and trimmed afterwards.
    global_batch: the inputs already ARE this rank's shard of a `global_batch`-image job (each rank
    generated / loaded only its own images); the shard sizes must then follow shard_bounds."""
    if global_batch is None:
        B = context[0].shape[0]
        lo, hi = shard_bounds(B, world_size, rank)
        sl = slice(lo, hi)
        rec = decode_fn(None if init is None else init[sl], [c[sl] for c in context])
    else:
        B = int(global_batch)
        lo, hi = shard_bounds(B, world_size, rank)
        if context[0].shape[0] != hi - lo:
            raise ValueError(f"rank {rank} holds {context[0].shape[0]} images, its shard of {B} is {hi - lo}")
        rec = decode_fn(init, list(context))
    if dist is None:                  # (a one-rank process group still runs the gather: bench.py under torchrun at N=1)
        return rec
    import torch
    maxn = -(-B // world_size)
    pad = torch.zeros((maxn,) + tuple(rec.shape[1:]), dtype=rec.dtype, device=rec.device)
    pad[: hi - lo] = rec
    parts = [torch.empty_like(pad) for _ in range(world_size)]
    dist.all_gather(parts, pad)
    out = []
    for r in range(world_size):
        rlo, rhi = shard_bounds(B, world_size, r)
        out.append(parts[r][: rhi - rlo])
    return torch.cat(out, dim=0)
