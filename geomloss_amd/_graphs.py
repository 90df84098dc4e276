"""Host-side helpers of launch-bound loops: the hipGraph cache and the garbage-collector settling.  They call no kernel of the library
themselves; ``hip.py`` re-exports both names.
"""

import torch


def settle_host():
    """For latency-critical loops (serving, benchmarks): one full Python garbage collection now, and its survivors moved out of the
    collector's reach (``gc.freeze()``).  The first generation-2 collection of a process that has imported torch walks ~1e6 objects
    and takes 30-40 ms; it fires once, a few thousand container allocations in, wherever the program happens to be — and while the
    host is stopped the launch queue of a 2 ms loss drains and the GPU idles (measured: profiles/r05_shard_stall.txt; this was the
    intermittent 2x outlier of the B = 32 shard of BASELINE configs[3]).  Call it after the warm-up of such a loop; bench.py does."""
    import gc
    gc.collect()
    gc.freeze()


class GraphCache:
    """Captures ``fn(*tensors) -> tuple of tensors`` into a hipGraph (``torch.cuda.CUDAGraph``) the first time a key is
    seen and replays it afterwards.  Everything ``fn`` launches — our C-ABI kernels included: they are issued on torch's
    current stream, which is the capture stream — becomes one graph launch.  Inputs are copied into static buffers,
    outputs are cloned out of them.  Small LRU: a graph pins its memory pool."""

    def __init__(self, capacity=8):
        self.capacity, self.entries = capacity, {}

    def run(self, key, fn, inputs):
        entry = self.entries.pop(key, None)
        if entry is None:
            static_in = [t.detach().clone() for t in inputs]
            side = torch.cuda.Stream(device=static_in[0].device)
            side.wait_stream(torch.cuda.current_stream(static_in[0].device))
            with torch.cuda.stream(side):      # warm-up outside capture (loads code objects, sizes the allocator pools)
                fn(*static_in)
            torch.cuda.current_stream(static_in[0].device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = fn(*static_in)
            entry = (graph, static_in, static_out)
            if len(self.entries) >= self.capacity:
                self.entries.pop(next(iter(self.entries)))
        else:
            for dst, src in zip(entry[1], inputs):
                dst.copy_(src)
        self.entries[key] = entry   # most recently used last
        entry[0].replay()
        return tuple(None if o is None else o.clone() for o in entry[2])
