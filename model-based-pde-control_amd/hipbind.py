"""What every ctypes binding of a C-ABI HIP library shares: opening and typing the library, the raw handle of torch's
current stream, the tensor-or-None pointer and the ``_check(rc)`` that turns a non-zero status into the module's error.

A binding module keeps its own ``LIB_PATH``, ``SYMBOLS`` (rows of ``(name, restype, argtypes)``, the ``*_last_error`` row
included), error class, ``_lib`` cache and a two-line ``load()``; it binds ``stream``, ``ptr`` and the result of
``checker`` directly to its own names, so a launch costs no Python call beyond the ones it made before.
torch is imported when the first library is opened, never at import time.
"""
import ctypes
import os



class Slabs(ctypes.Structure):
    """``replay_slabs`` of include/replay/slabs.h: the seven slab pointers of a device-resident replay and their row
    count.  The C headers alias it as ``rp_slab``, ``ks_record`` and ``bg_slabs``; the bindings as ``replay_hip.Slab``,
    ``kspde.ks_record`` and ``pdegym.burgers._hip.Slabs``."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("obs", "actions", "nxtobs", "rewards", "terminated", "truncated", "steps")] \
        + [("rows", ctypes.c_long)]


_torch = None       # the torch module, once open_library has imported it (nothing launches before a library is open)


def open_library(path, symbols, error, no_fallback):
    """dlopen ``path`` and type every row of ``symbols``.  A missing file raises ``error`` (path, build hint, then the
    module's ``no_fallback`` sentence); a symbol the library lacks raises AttributeError."""
    if not os.path.exists(path):
        raise error(f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                    f"g.build()' or make -C model-based-pde-control_amd/csrc). {no_fallback}")
    # torch ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  Import it
    # FIRST so that the library's NEEDED libamdhip64.so.7 binds to that already-loaded copy: two HIP
    # runtimes in one process cannot both own the GPU ("No HIP GPUs are available").
    global _torch
    import torch
    _torch = torch
    return type_symbols(ctypes.CDLL(path), symbols)


def type_symbols(lib, symbols):
    """Set restype and argtypes of every row of ``symbols`` on the open library ``lib`` (a second table over a library
    another module opened: the ``fno_*`` half of libspectral_hip) and return it."""
    for name, res, args in symbols:
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    return lib


def stream():
    # raw handle of torch's current stream; torch.cuda.current_stream() costs ~8 us of Python per call and the eager
    # step makes a dozen
    return ctypes.c_void_p(_torch._C._cuda_getCurrentRawStream(_torch.cuda.current_device()))


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def checker(error, label, last_error, load):
    """The module's ``_check(rc)``: on a non-zero status raises ``error("<label> error <rc>: <text>")`` with the text of
    the library's ``last_error`` symbol.  ``load`` is called only then (pass ``lambda: load()`` so that the module's
    ``load`` is looked up at that moment)."""
    def check(rc):
        if rc != 0:
            raise error(f"{label} error {rc}: {getattr(load(), last_error)().decode(errors='replace')}")
    return check
