"""Recording the C-ABI launches of real train steps (shared by tests/test_gpu_step_replay.py and
tests/test_gpu_step_glue_replay.py).

One or more train steps run with the library handle swapped for a Recorder (as scripts/conv_shapes.py does).  Every call
of an entry point that `want(name)` accepts is split by its argument names (a spec table: name -> (family, argument
names in C order); the names in `ptrs` are pointers, every other one a number) into

    ints    the numeric arguments (integers as int, float arguments as float),
    nulls   NULL / non-NULL of every pointer argument but the stream,
    aligns  (only with align=True) the address modulo 16 of every non-NULL pointer argument that is a plain device
            pointer -- the replay builds its operands at the same misalignment (a storage offset into a larger buffer),
    extra   (only with align=True) what `extra[name](args)` returns: the NULL pattern of host pointer arrays, the
            non-pointer fields of a device descriptor table (read_device), aliasing of two arguments ...

and deduplicated by that key."""
import collections
import ctypes

import torch

DEV = "cuda:0"


def is_null(v):
    if v is None:
        return True
    if isinstance(v, ctypes.c_void_p):
        return not v.value
    return False


def address(v):
    """The address a pointer argument holds (None: not a plain device pointer -- a host array)."""
    if isinstance(v, ctypes.c_void_p):
        return v.value or 0
    if isinstance(v, int):
        return v
    return None


def _num(v):
    if isinstance(v, (ctypes.c_float, ctypes.c_double)):
        return float(v.value)
    if isinstance(v, float):
        return float(v)
    if isinstance(v, (ctypes.c_int, ctypes.c_long, ctypes.c_size_t)):
        return int(v.value)
    return int(v)


_HIP = None


def read_device(addr, nbytes):
    """Bytes at a raw device address (a descriptor table the step built), copied to the host after a device-wide
    synchronisation."""
    global _HIP
    if _HIP is None:
        import os
        # the HIP runtime torch itself loaded (one runtime per process)
        _HIP = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(nbytes)
    rc = _HIP.hipMemcpy(buf, ctypes.c_void_p(addr), ctypes.c_size_t(nbytes), 2)     # hipMemcpyDeviceToHost
    assert rc == 0, "hipMemcpy from a recorded descriptor table failed (%d)" % rc
    return buf.raw


class Recorder(object):
    """Stands in for the CDLL: the entry points `want` accepts log their record key into `records` (an ordered dict);
    an accepted name missing from `specs` is logged as (name, (), ()) so that the test can report it."""

    def __init__(self, real, records, want, specs, ptrs, align=False, extra=None):
        self._real = real
        self._records = records
        self._want = want
        self._specs = specs
        self._ptrs = ptrs
        self._align = align
        self._extra = extra or {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not self._want(name):
            return fn
        _, args = self._specs.get(name, (None, None))
        ptrs = self._ptrs

        def rec(*a):
            if args is None:
                self._records[(name, (), ())] = None
                return fn(*a)
            ints = tuple((k, _num(v)) for k, v in zip(args, a) if k not in ptrs)
            nulls = tuple((k, is_null(v)) for k, v in zip(args, a) if k in ptrs and k != "stream")
            if not self._align:
                self._records[(name, ints, nulls)] = None
                return fn(*a)
            aligns = tuple((k, address(v) % 16) for k, v in zip(args, a)
                           if k in ptrs and k != "stream" and not is_null(v) and address(v) is not None)
            ex = self._extra.get(name)
            info = ex(dict(zip(args, a))) if ex is not None else ()
            self._records[(name, ints, nulls, aligns, info)] = None
            return fn(*a)
        return rec


def record_step(cfg_kw, size, batch_size, want, specs, ptrs, steps=2, align=False, extra=None, around=None):
    """Builds the model of `cfg_kw` (seeded as the headline test does), runs `steps` train steps with the recorder in
    place and returns (list of record keys, model).  `around(model, opt)` may return a context manager that wraps the
    steps (the SGD check of the glue replay)."""
    import contextlib
    from feature_intertwiner_amd import _lib
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    from feature_intertwiner_amd.workflow import set_optimizer, train_step
    torch.manual_seed(2000)
    cfg = make_config(**cfg_kw)
    model = MaskRCNN(cfg).to(DEV)
    opt = set_optimizer(model, cfg.TRAIN)
    batch = synthetic_batch(batch_size, size, device=DEV, seed=2000)
    model.external_proposals = SyntheticProposals(batch[2], size, seed=7)
    model.generator = torch.Generator(device=DEV).manual_seed(11)
    records = collections.OrderedDict()
    real = _lib.load()
    _lib._lib = Recorder(real, records, want, specs, ptrs, align=align, extra=extra)
    try:
        with (around(model, opt) if around is not None else contextlib.nullcontext()):
            for _ in range(steps):
                terms = train_step(model, opt, list(batch))
            torch.cuda.synchronize()
    finally:
        _lib._lib = real
    assert all(torch.isfinite(v) for v in terms.values()), terms
    del opt, batch
    torch.cuda.empty_cache()
    return list(records), model
