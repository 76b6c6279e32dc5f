"""HIP-backed counterpart of the variant ``TransducerGRU``.

Mirrors /root/reference/pepper_variant/modules/python/models/simple_model.py:6-87: same
constructor arguments, same state_dict keys/shapes, ``forward(x, train_mode=False)`` returning
softmax probabilities [B,3] (logits when ``train_mode``).  All arithmetic runs in
libpepper_amd.so on the GPU; torch is used only for device memory and stream ordering.
"""
import torch

from pepper_amd import _lib
from pepper_amd._handle import NEW_HANDLES, HandleModel, _pinned_empty  # noqa: F401  (NEW_HANDLES: set by variant/fused.py)
from pepper_amd.variant.Options import ImageSizeOptions


class TransducerGRU(HandleModel):
    KIND = "variant"

    def __init__(self, image_features, gru_layers, hidden_size, num_classes, num_classes_type,
                 bidirectional=True, device=None, max_chunk=0, batch_invariant=None):
        if not bidirectional:
            raise ValueError("the reference inference path only instantiates bidirectional=True")
        HandleModel.__init__(self, device, max_chunk, batch_invariant)
        self.image_features = image_features
        self.hidden_size = hidden_size          # kept for parity; layer widths are fixed at 256/512
        self.bidirectional = bidirectional
        self.num_layers = gru_layers
        self.num_classes = num_classes
        self.num_classes_type = num_classes_type
        self.window = ImageSizeOptions.CANDIDATE_WINDOW_SIZE + 1

    # ---- nn.Module-like surface used by predict() (the rest of it: HandleModel) ------------------
    def load_state_dict(self, state_dict, strict=True):
        return self._create(_lib.VariantConfig(self.image_features, self.window, self.num_layers,
                                               self.num_classes_type, self.device, self.max_chunk), state_dict)

    def __call__(self, x, train_mode=False):
        return self.forward(x, train_mode)

    def forward(self, x, train_mode=False):
        """x: [B, 33, 26] int8 (as stored in the images HDF5) or float tensor, CPU or GPU."""
        lib = _lib.load()
        x = torch.as_tensor(x)
        if x.dim() != 3 or x.shape[1] != self.window or x.shape[2] != self.image_features:
            raise ValueError(f"expected [B,{self.window},{self.image_features}], got {tuple(x.shape)}")
        on_cpu = not x.is_cuda
        dev = torch.device("cuda", self.device)
        if on_cpu and x.dtype == torch.int8:
            # host buffers (what the predict loop hands over: a file's packed int8 windows, page-locked): device passes
            # with the H2D copy of the next pass and the D2H copy of the previous one beside the kernels
            x = x.contiguous()
            n = x.shape[0]
            probs = _pinned_empty((n, self.num_classes_type), torch.float32)
            logits = _pinned_empty((n, self.num_classes_type), torch.float32) if train_mode else None
            _lib.check(lib.pa_variant_forward_host(self.handle, x.data_ptr(), n, probs.data_ptr(),
                                                   logits.data_ptr() if logits is not None else None))
            return logits if train_mode else probs
        if x.dtype not in (torch.int8, torch.float32):
            x = x.to(torch.float32)
        x = x.to(dev).contiguous()
        n = x.shape[0]
        probs = torch.empty((n, self.num_classes_type), dtype=torch.float32, device=dev)
        logits = torch.empty_like(probs) if train_mode else None
        fn = lib.pa_variant_forward_device if x.dtype == torch.int8 else lib.pa_variant_forward_device_f32
        with self._on_stream(x, probs, logits):
            _lib.check(fn(self.handle, x.data_ptr(), n, probs.data_ptr(),
                          logits.data_ptr() if logits is not None else None))
        out = logits if train_mode else probs
        return out.cpu() if on_cpu else out
