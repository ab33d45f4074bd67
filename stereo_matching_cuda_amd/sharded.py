"""Disparity-slice sharding across ranks (one process per GPU) and the one exchange step of the
path: a per-pixel MIN all-reduce of packed (cost, slice) keys (RCCL over xGMI with backend "nccl",
gloo on CPU).  No reference counterpart (the reference is single-GPU); SURVEY.md 8e.

Rank g of G owns the contiguous slice range [g*D//G, (g+1)*D//G) of BOTH volumes; the two gray
images are replicated and the guidance statistics recomputed per rank (deterministic, bit-equal).
The signed min of the packed keys is exactly the sequential `best >= q` rule of dispSelectOnGPU
(guidedFilter.cu:403-411): smallest cost, and among equal costs the largest slice.
"""
import numpy as np
import torch
import torch.distributed as dist


def shard_range(size_d, rank, world):
    """Contiguous, balanced, possibly empty slice range of `rank`."""
    return (rank * size_d) // world, ((rank + 1) * size_d) // world


def allreduce_min_keys_(keys_i64, group=None):
    """In-place MIN all-reduce of packed int64 keys (the kernels emit them in signed order, so this
    is the collective and nothing else).  Device tensors go through RCCL (backend "nccl"); with a
    gloo group (CPU rehearsal of the N>1 path, several ranks sharing one GPU) they are staged
    through host memory."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        if keys_i64.is_cuda and dist.get_backend(group) == "gloo":
            host = keys_i64.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.MIN, group=group)
            keys_i64.copy_(host)
        else:
            dist.all_reduce(keys_i64, op=dist.ReduceOp.MIN, group=group)
    return keys_i64


def merge_keys_host(key_arrays):
    """Reference merge for tests: elementwise signed min over a list of numpy int64 arrays."""
    out = np.asarray(key_arrays[0], dtype=np.int64).copy()
    for k in key_arrays[1:]:
        np.minimum(out, np.asarray(k, dtype=np.int64), out=out)
    return out


class ShardedPair:
    """D-sharded stereo pair: local aggregation of this rank's slices, ONE all-reduce of both
    views' keys, then decode + LR check + filling (replicated on every rank: n-sized, microseconds).
    The census and AD-Census matching costs (PairPipeline(cost="census" / "adcensus")) are not part of the sharded driver:
    cost=... raises ValueError.  Neither is speckle removal (PairPipeline(speckle=...)): speckle=... raises ValueError, and so
    do region voting (PairPipeline(vote=...)) and the depth-discontinuity adjustment (PairPipeline(adjust=...)).  Nor is semi-global matching, which needs a pixel's whole disparity range on
    one rank: aggregation="sgm" and aggregation="bp" raise ValueError, and so do the scan-line optimiser's "scanline" / "cross-scanline"."""

    def __init__(self, w, h, size_d, rank=0, world=1, group=None, **kw):
        from .device import PairPipeline
        if world > 1 and kw.get("subpixel") is not None:
            # the neighbours of a winner at a shard boundary were aggregated on another rank
            raise ValueError("subpixel needs the whole slice range on one rank (world == 1)")
        if kw.get("cost") is not None:
            raise ValueError("the census and AD-Census costs are not part of the sharded driver: use "
                             f"PairPipeline(cost={kw['cost']!r})")
        if kw.get("speckle") is not None:
            raise ValueError("speckle removal is not part of the sharded driver: use PairPipeline(speckle=...)")
        if kw.get("vote") is not None or kw.get("vote_arms") is not None:
            raise ValueError("region voting is not part of the sharded driver: use PairPipeline(vote=...)")
        if kw.get("adjust") is not None:
            # (a D-shard holds no whole aggregated volume)
            raise ValueError("the depth-discontinuity adjustment is not part of the sharded driver: use PairPipeline(adjust=...)")
        if kw.get("permeability") is not None:
            # (the filter runs over whole aggregated volumes)
            raise ValueError("the permeability filter is not part of the sharded driver: use PairPipeline(permeability=...)")
        if kw.get("cross_scale") is not None:
            # (the combination reads whole volumes of every level)
            raise ValueError("cross-scale aggregation is not part of the sharded driver: use PairPipeline(cross_scale=...)")
        if kw.get("aggregation") in ("scanline", "cross-scanline") or kw.get("scanline_params") is not None:
            raise ValueError("the scan-line optimiser is not part of the sharded driver: use "
                             f"PairPipeline(aggregation={kw.get('aggregation')!r})")
        if kw.get("aggregation") == "patchmatch" or kw.get("pm_params") is not None:
            # (there are no slices to shard: the search has no cost volume)
            raise ValueError("PatchMatch stereo is not part of the sharded driver: use PairPipeline(aggregation='patchmatch')")
        if kw.get("aggregation") == "bp" or kw.get("bp_params") is not None:
            # (a message needs every label of a pixel: there are no slices to shard)
            raise ValueError("belief propagation is not part of the sharded driver: use PairPipeline(aggregation='bp')")
        if kw.get("aggregation") is not None:
            raise ValueError("semi-global matching is not part of the sharded driver: use PairPipeline(aggregation='sgm')")
        self.rank, self.world, self.group = rank, world, group
        s0, s1 = shard_range(size_d, rank, world)
        self.pipe = PairPipeline(w, h, size_d, s_begin=s0, s_end=s1, **kw)

    def run(self, gray_l, gray_r):
        self.pipe.aggregate(gray_l, gray_r)
        if self.world > 1:
            allreduce_min_keys_(self.pipe.keys, self.group)
        self.pipe.finish()
        return self.pipe
