"""The cache of reused permutations of the sorted p = 2 call: its key and its container.  Pure Python on tensor metadata; the instance,
the plan of a call (``_perm_plan``) and everything that touches the library stay in ``hip.py``, which re-exports these names.
"""

import collections
import threading

PERM_CACHE_ENTRIES = 8


def perm_cache_key(t, stream_id):
    """The key under which the sorted order of the cloud ``t`` ((N,D) or (1,N,D)) is kept: the identity of its storage, its data pointer,
    the shape and strides of its last two axes, dtype, device, the launch stream and the tensor's version counter.  Pure Python on
    tensor metadata (CPU tensors have keys too).  ``.detach()`` and views share storage and counter, so ``x``, ``x.detach()`` and
    ``x[None]`` have one key; an in-place torch write bumps the counter.  None: a tensor without a counter (inference mode)."""
    try:
        version = t._version
    except RuntimeError:
        return None
    return (t.untyped_storage()._cdata, t.data_ptr(), tuple(t.shape[-2:]), tuple(t.stride()[-2:]), t.dtype, str(t.device),
            int(stream_id), int(version))


class _PermCache:
    """Per-CLOUD cache of the int32 permutations that ``glhip_sinkhorn_step_perm`` exports and takes back as hints.

    The sorted p = 2 call (``softmin_perm_applies``: one dense problem of D <= 3 and N M >= 1e11) orders each cloud by its coordinates
    alone — bounding box, voxel path keys, a 64-bit radix sort, balanced cells — before anything that depends on the dual vector or the
    temperature.  A Sinkhorn loss calls 4 x (n_eps + 2) times on the same two clouds, and a cloud has the same order as rows and as
    columns, so ``(x, y)``, ``(y, x)``, ``(x, x)`` and ``(y, y)`` share two entries: two sorts per loss.  Everything that depends on
    ``h`` or ``eps`` — the gathers of the vectors, the three pruning kernels, the reduction — runs on every call.

    An entry is used only if every part of :func:`perm_cache_key` matches and the storage is alive (a weak reference to the storage,
    not to the Python tensor: the drivers pass fresh ``.detach()`` / ``[None]`` views on every call).  Entries of dead storages are
    dropped at every lookup, which frees their permutations; a fresh tensor on a freed address is another storage and misses; another
    stream misses (the permutation was produced elsewhere); at most ``PERM_CACHE_ENTRIES`` entries, least recently used out.
    While the current stream is capturing a graph the cache is neither read nor filled: a replay must not depend on a buffer that the
    cache may free.

    What the key does NOT see: writes that bypass the version counter — through ``.data``, a raw pointer, another library.  The entry
    is then stale, and the result is STILL RIGHT: the pruning is exact for any order (csrc/glhip_autosort.h), every box it uses is
    recomputed from the gathered coordinates on every call, and a stale order only keeps more pairs, that is, costs time.
    ``hip.forget_permutations`` clears the cache; ``GEOMLOSS_HIP_PERM_CACHE=0`` turns it off."""

    def __init__(self):
        self.lock = threading.Lock()
        self.entries = collections.OrderedDict()      # key -> (StorageWeakRef, permutation)
        self.hits = self.misses = 0

    def lookup(self, key):
        """The permutation kept for ``key`` (counted as a hit), or None (a miss); drops the entries of dead storages."""
        with self.lock:
            for k in [k for k, (ref, _) in self.entries.items() if ref.expired()]:
                del self.entries[k]
            hit = self.entries.get(key)
            if hit is None:
                self.misses += 1
                return None
            self.entries.move_to_end(key)
            self.hits += 1
            return hit[1]

    def store(self, key, t, perm):
        from torch.multiprocessing.reductions import StorageWeakRef
        with self.lock:
            self.entries[key] = (StorageWeakRef(t.untyped_storage()), perm)
            self.entries.move_to_end(key)
            while len(self.entries) > PERM_CACHE_ENTRIES:
                self.entries.popitem(last=False)

    def clear(self):
        with self.lock:
            self.entries.clear()
