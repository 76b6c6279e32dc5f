"""What the two HIP-backed ``TransducerGRU`` wrappers (variant/models/simple_model.py, polish/models/simple_model.py) share:
the life of a libpepper_amd.so model handle and of the stream it runs on."""
import contextlib
import ctypes
import threading

import torch

from pepper_amd import _lib


def _pinned_empty(shape, dtype):
    """Page-locked result buffer (the D2H copies of the host entry points are asynchronous only into pinned memory);
    falls back to pageable memory where pinning is refused."""
    try:
        return torch.empty(shape, dtype=dtype, pin_memory=True)
    except RuntimeError:
        return torch.empty(shape, dtype=dtype)


# Per thread: the priority of the stream a handle made on this thread gets (0; -1 = one of the device's high-priority queues).  The
# loaders keep the reference's signatures, so a caller that wants its forwards not to queue behind other streams' long kernels in a
# shared hardware queue (variant/fused.py; polish/fused.py through clone()) sets NEW_HANDLES.stream_priority around its load.
NEW_HANDLES = threading.local()


class HandleModel(object):
    """nn.Module-like shell around one pa_<KIND>_model handle."""
    KIND = None   # "variant" / "polish": the handle's entry points are pa_<KIND>_create / _destroy / _set_batch_invariant / ...

    def __init__(self, device, max_chunk, batch_invariant):
        self.max_chunk = max_chunk
        # batch-invariant mode (include/pepper_amd.h pa_*_set_batch_invariant): on when asked for here, or when the process
        # has PEPPER_AMD_BATCH_INVARIANT=1
        # and the argument is left at None (an explicit True / False wins over the environment)
        self.batch_invariant = _lib.batch_invariant_default(batch_invariant)
        self.device = torch.cuda.current_device() if device is None and torch.cuda.is_available() else (device or 0)
        self._handle = None
        self._stream = None
        self.training = False

    def _entry(self, name):
        return getattr(_lib.load(), f"pa_{self.KIND}_{name}")

    def _create(self, cfg, state_dict):
        """A new handle on its own stream (this one's, if any, is closed first), in the mode the object was made with."""
        self.close()
        names, data, numel, n, keep = _lib.marshal_state_dict(state_dict)
        self._stream = torch.cuda.Stream(device=self.device, priority=int(getattr(NEW_HANDLES, "stream_priority", 0)))
        handle = ctypes.c_void_p()
        _lib.check(self._entry("create")(ctypes.byref(cfg), names, data, numel, n,
                                         ctypes.c_void_p(self._stream.cuda_stream), ctypes.byref(handle)))
        self._handle = handle
        if self.batch_invariant:
            try:
                _lib.check(self._entry("set_batch_invariant")(handle, 1))
            except _lib.PepperAmdError:
                self.close()             # (polish's exact-f32 kernels refuse the mode: no handle without the guarantee asked for)
                raise
        return self

    def set_batch_invariant(self, on=True):
        """Switch the handle's batch-invariant mode between calls (it applies from the next forward / prediction)."""
        on = _lib.parse_batch_invariant(on)
        _lib.check(self._entry("set_batch_invariant")(self.handle, int(on)))
        self.batch_invariant = on
        return self

    def get_batch_invariant(self):
        v = ctypes.c_int32()
        _lib.check(self._entry("get_batch_invariant")(self.handle, ctypes.byref(v)))
        return bool(v.value)

    @contextlib.contextmanager
    def _on_stream(self, *tensors):
        """Bracket of a device entry point: the handle's stream waits for what the caller's current stream has queued, the
        tensors the call touches (None entries skipped) are kept alive for the handle's stream, and the caller's stream
        waits for the call's kernels."""
        cur = torch.cuda.current_stream(torch.device("cuda", self.device))
        self._stream.wait_stream(cur)
        yield
        for t in tensors:
            if t is not None:
                t.record_stream(self._stream)
        cur.wait_stream(self._stream)

    def eval(self):
        self.training = False
        return self

    def cuda(self, device=None):
        return self

    def cpu(self):
        return self

    def close(self):
        if self._handle is not None:
            self._entry("destroy")(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        if self._handle is None:
            raise _lib.PepperAmdError("TransducerGRU has no weights: call load_state_dict first")
        return self._handle
