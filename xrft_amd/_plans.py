"""What the API keeps between calls about plans: digests of host arrays, the plan cache, the descriptors the library declined, the two-stage decisions."""
from __future__ import annotations

import threading
from collections import OrderedDict

import numpy as np

from . import _lib, engine

_plan_lock = threading.RLock()  # the functions are pure like the reference's: callable from several (dask-style) worker threads

# Host work that depends only on (length, spacing) or on a coordinate vector is memoised: the reference recomputes it on
# every call, here it would be most of the ~0.25 ms a call costs on the host (what small problems are made of).
_memo = {}
_memo_ids = {}  # id(memoised vector) -> its key: plans are keyed by it instead of by a hash of 32 KB of window samples

try:  # bytes -> 64-bit digest at ~10 GB/s (python's own bytes hash does 2 GB/s: 16 us per 4096-point coordinate)
    import xxhash

    def _digest(arr):
        return xxhash.xxh3_64_intdigest(np.ascontiguousarray(arr))
except Exception:  # pragma: no cover
    def _digest(arr):
        return hash(np.ascontiguousarray(arr).tobytes())


def _memoised(key, fn):
    with _plan_lock:
        hit = _memo.get(key)
    if hit is None:
        hit = fn()
        with _plan_lock:
            if len(_memo) > 512:
                _memo.clear()
                _memo_ids.clear()
            _memo[key] = hit
            if isinstance(hit, np.ndarray):
                _memo_ids[id(hit)] = key
    return hit


def _ro(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


_plan_cache: "OrderedDict[tuple, engine.SpectralPlan]" = OrderedDict()
_PLAN_CACHE_SIZE = 16


_digest_ids = {}  # id(read-only array) -> (the array, its digest): tables that are built once per labelled array (phase factors,
#                   coordinate vectors) are digested once, not on every call (1 MB of phase factors per 65536-point axis: 100 us)


def _akey(a):
    if a is None:
        return None
    k = _memo_ids.get(id(a))  # a memoised window vector: identified by (name, n)
    if k is not None:
        return k
    if a.flags.writeable or not a.flags.owndata or a.base is not None:  # (a read-only VIEW of a writeable base can change under its id)
        return _digest(a)
    with _plan_lock:
        e = _digest_ids.get(id(a))
    if e is not None and e[0] is a:
        return e[1]
    d = _digest(a)
    with _plan_lock:
        if len(_digest_ids) > 256:
            _digest_ids.clear()
        _digest_ids[id(a)] = (a, d)
    return d


def _plan_key(binmap_key, kw):
    # the bin map can be 16M entries: it is identified by the key of the (cached) host computation, not by its bytes
    return (engine.bluestein_in_float64(),) + tuple((k, (binmap_key if k == "binmap" else _akey(v)) if isinstance(v, np.ndarray) else v)
                                                    for k, v in sorted(kw.items()))


def _get_plan(binmap_key=None, **kw):
    return _plan_for(_plan_key(binmap_key, kw), kw)  # (the key includes the input strides of a plan that reads a view where it lies)


def _plan_for(key, kw):
    with _plan_lock:
        p = _plan_cache.get(key)
        if p is None:
            p = engine.SpectralPlan(**kw)
            _plan_cache[key] = p
            while len(_plan_cache) > _PLAN_CACHE_SIZE:
                _plan_cache.popitem(last=False)
        else:
            _plan_cache.move_to_end(key)
    return p


class _DeclinedKeys:
    """Plan keys the library answered XRFTHIP_UNSUPPORTED_LENGTH to: a bounded set in insertion order, the oldest key goes first."""

    def __init__(self, capacity=64):
        self._keys, self._capacity = OrderedDict(), capacity

    def __len__(self):
        return len(self._keys)

    def __contains__(self, key):
        with _plan_lock:
            return key in self._keys

    def add(self, key):
        with _plan_lock:
            self._keys[key] = True
            while len(self._keys) > self._capacity:
                self._keys.popitem(last=False)

    def clear(self):
        with _plan_lock:
            self._keys.clear()


_MEAN_REFUSED = _DeclinedKeys()     # ... with mean_batch: those calls compose (the plain plan, then .mean), without asking again
_STRIDED_REFUSED = _DeclinedKeys()  # ... with input strides: those calls copy, without asking again
_HALF_REFUSED = _DeclinedKeys()     # ... with float16 / bfloat16 input: those calls widen the field once (engine.convert) and take the float32 plan


def _rung(declined, binmap_key, kw, run=None, key=None):
    """One rung of the ladder of plans: the cached plan of the descriptor ``kw`` -- or, with ``run``, what ``run(plan)`` returns -- else None, once the library has
    answered XRFTHIP_UNSUPPORTED_LENGTH; the refusal is remembered in ``declined`` and the library is not asked again.  ``run`` stays inside the ``try``: xrfthip_exec
    of a half plan answers UNSUPPORTED_LENGTH too (a field that is not 16-byte aligned, a family without a half loader).  ``key``: the plan key where the caller
    has it already.  Every other error propagates."""
    if key is None:
        key = _plan_key(binmap_key, kw)
    if key in declined:
        return None
    try:
        plan = _plan_for(key, kw)
        return plan if run is None else run(plan)
    except _lib.XrftHipError as e:
        if e.status != _lib.UNSUPPORTED_LENGTH:
            raise
        declined.add(key)
        return None


_TWO_STAGE = OrderedDict()  # _ifft_two_stages: (shape, flags, tables) -> bool, a small LRU of DECISIONS (the stage plans live in _plan_cache only:
_TWO_STAGE_SIZE = 32                   # its LRU governs their lifetime and their device tables)
