"""Training-input preprocessing on the GPU: the reference loader's TrainPre / ValPre
(utils/dataloader/dataloader.py:20-76, 112-122) for a whole batch of raw uint8 images in one kernel launch.

    pre = TrainPre(norm_mean, norm_std, (480, 640), scales, modal_mean, modal_std)
    params = pre.draw(B, (H0, W0), random)                       # host: mirror, scale, crop position per sample
    rgb, modal, label = pre(rgb_u8, modal_u8, gt_u8, params)     # device: [B,3,ch,cw] f32, [B,Cm,ch,cw] f32, [B,ch,cw] i64
    pre(rgb_u8, modal_u8, gt_u8, params, out=graphed_step.inputs)  # or straight into a model's static buffers

This module binds libdformer_data.so (include/dformer_data.h), a library of its own: nothing else in the
package imports it, so `import dformer_amd` and the training path map the model library alone. There is no
torch fallback: a missing library is an ImportError.
"""
import ctypes
import numbers
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdformer_data.so")

MAX_DIM, MAX_SCALED = 16384, 32768  # DFD_MAX_DIM, DFD_MAX_SCALED
c_int, c_float, P = ctypes.c_int, ctypes.c_float, ctypes.c_void_p


class PreDesc(ctypes.Structure):
    """DfdPreDesc."""
    _fields_ = [("B", c_int), ("H0", c_int), ("W0", c_int), ("ch", c_int), ("cw", c_int), ("modal_channels", c_int),
                ("bgr", c_int), ("transform_gt", c_int), ("mean", c_float * 3), ("std", c_float * 3),
                ("modal_mean", c_float * 3), ("modal_std", c_float * 3)]


# name -> (restype, argtypes)
_SIGS = {
    "dfd_last_error": (ctypes.c_char_p, []),
    "dfd_abi_version": (c_int, []),
    "dfd_train_pre": (c_int, [ctypes.POINTER(PreDesc), P, P, P, P, P, P, P, P]),
}

ABI_VERSION = 1  # the dfd_abi_version() PreDesc and _SIGS were written for


def check_abi(lib):
    got = lib.dfd_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"dformer_amd.data: {LIB_PATH} has ABI version {got}, these bindings expect {ABI_VERSION}; "
                          f"rebuild it from this tree's csrc")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"dformer_amd.data: native library missing at {LIB_PATH}; run "
                          f"`python -c 'import __graft_entry__ as g; g.build()'` (make -C dformer_amd/csrc)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    check_abi(lib)
    return lib


lib = _load()


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what} failed ({status}): {lib.dfd_last_error().decode()}")


def _triple(v, what):
    vals = [float(v)] if isinstance(v, numbers.Real) else [float(x) for x in v]
    if len(vals) == 1:
        vals = vals * 3
    if len(vals) != 3:
        raise ValueError(f"{what}: want a number or 1 or 3 values, got {len(vals)}")
    return vals


def check_params(params, B):
    """Range-check a host parameter tensor: int32 [B,8] rows (flip, sh, sw, pos_h, pos_w, 0, 0, 0)."""
    if params.dtype != torch.int32 or tuple(params.shape) != (B, 8):
        raise ValueError(f"params: want int32 [{B}, 8], got {params.dtype} {tuple(params.shape)}")
    for b, (flip, sh, sw, pos_h, pos_w, *rest) in enumerate(params.tolist()):
        if flip not in (0, 1):
            raise ValueError(f"params[{b}]: flip {flip}, want 0 or 1")
        if not (0 <= sh <= MAX_SCALED and 0 <= sw <= MAX_SCALED):
            raise ValueError(f"params[{b}]: scaled size {sh} x {sw} outside 0..{MAX_SCALED}")
        if pos_h < 0 or pos_w < 0 or (sh > 0 and pos_h >= sh) or (sw > 0 and pos_w >= sw):
            raise ValueError(f"params[{b}]: crop position ({pos_h}, {pos_w}) outside the scaled image {sh} x {sw}")
        if any(rest):
            raise ValueError(f"params[{b}]: columns 5..7 are reserved and must be 0")


class _Pre:
    def __init__(self, norm_mean, norm_std, modal_mean, modal_std, transform_gt, bgr):
        self.mean, self.std = _triple(norm_mean, "norm_mean"), _triple(norm_std, "norm_std")
        self.modal_mean = self.mean if modal_mean is None else _triple(modal_mean, "modal_mean")
        self.modal_std = self.std if modal_std is None else _triple(modal_std, "modal_std")
        if min(self.std + self.modal_std) <= 0:
            raise ValueError("norm_std / modal_std must be > 0")
        self.transform_gt, self.bgr = bool(transform_gt), bool(bgr)

    def _run(self, rgb_u8, modal_u8, gt_u8, params, crop, out):
        """params: int32 [B,8] on the inputs' device. Enqueues one kernel on the current stream."""
        if rgb_u8.dim() != 4 or rgb_u8.shape[3] != 3:
            raise ValueError(f"rgb_u8: want [B,H0,W0,3], got {tuple(rgb_u8.shape)}")
        B, H0, W0, _ = rgb_u8.shape
        one_size = "one raw size H0 x W0 per call: a batch of samples with different raw sizes is not supported"
        if tuple(modal_u8.shape) not in ((B, H0, W0), (B, H0, W0, 3)):
            raise ValueError(f"modal_u8: want [{B},{H0},{W0}] or [{B},{H0},{W0},3], got {tuple(modal_u8.shape)} ({one_size})")
        if tuple(gt_u8.shape) != (B, H0, W0):
            raise ValueError(f"gt_u8: want [{B},{H0},{W0}], got {tuple(gt_u8.shape)} ({one_size})")
        dev = rgb_u8.device
        for name, t in (("rgb_u8", rgb_u8), ("modal_u8", modal_u8), ("gt_u8", gt_u8)):
            if t.dtype != torch.uint8 or not t.is_cuda or t.device != dev or not t.is_contiguous():
                raise ValueError(f"{name}: want a contiguous uint8 tensor on {dev}")
        if params.dtype != torch.int32 or tuple(params.shape) != (B, 8) or params.device != dev or \
                not params.is_contiguous():
            raise ValueError(f"params: want a contiguous int32 [{B}, 8] tensor on {dev}")
        cm = 1 if modal_u8.dim() == 3 else 3
        ch, cw = crop
        shapes = ((B, 3, ch, cw), (B, cm, ch, cw), (B, ch, cw))
        dtypes = (torch.float32, torch.float32, torch.int64)
        if out is None:
            out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
        else:
            out = tuple(out)
            if len(out) != 3:
                raise ValueError("out: want (rgb, modal, label)")
            for name, t, s, d in zip(("rgb", "modal", "label"), out, shapes, dtypes):
                if tuple(t.shape) != s or t.dtype != d or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"out {name}: want a contiguous {d} {list(s)} tensor on {dev}, got {t.dtype} "
                                     f"{list(t.shape)} on {t.device}")
        desc = PreDesc(B, H0, W0, ch, cw, cm, int(self.bgr), int(self.transform_gt), (c_float * 3)(*self.mean),
                       (c_float * 3)(*self.std), (c_float * 3)(*self.modal_mean), (c_float * 3)(*self.modal_std))
        with torch.cuda.device(dev):
            check(lib.dfd_train_pre(desc, rgb_u8.data_ptr(), modal_u8.data_ptr(), gt_u8.data_ptr(), params.data_ptr(),
                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), "dfd_train_pre")
        return out


class TrainPre(_Pre):
    """The reference's TrainPre on the device. crop_size = (image_height, image_width), scales =
    config.train_scale_array (None: no rescaling). modal_mean / modal_std default to the rgb values (the
    reference's sign=False); a 1-channel modal uses their first element. transform_gt stores (g - 1) & 255
    (RGBXDataset._gt_transform); bgr reads the rgb (and a 3-channel modal) source as cv2.imread returns it."""

    def __init__(self, norm_mean, norm_std, crop_size, scales, modal_mean=None, modal_std=None, transform_gt=False,
                 bgr=False):
        super().__init__(norm_mean, norm_std, modal_mean, modal_std, transform_gt, bgr)
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        self.scales = None if scales is None else list(scales)

    def draw(self, B, raw_hw, rng):
        """The per-sample random choices in the reference's order, from a random.Random-like `rng`:
        random() >= 0.5 mirrors; choice(scales) if scales is given; randint(0, sh - ch + 1) only if the scaled
        image is taller than the crop, likewise for the width (randint includes its upper end, so a crop may
        start one row late and end in one padded row: generate_random_crop_pos, transforms.py:44-59).
        Returns int32 [B,8] rows (flip, sh, sw, pos_h, pos_w, 0, 0, 0), pinned where a GPU is present."""
        H0, W0 = raw_hw
        ch, cw = self.crop_size
        rows = []
        for _ in range(B):
            flip = int(rng.random() >= 0.5)
            sh, sw = H0, W0
            if self.scales is not None:
                s = rng.choice(self.scales)
                sh, sw = int(H0 * s), int(W0 * s)
            pos_h = rng.randint(0, sh - ch + 1) if sh > ch else 0
            pos_w = rng.randint(0, sw - cw + 1) if sw > cw else 0
            rows.append([flip, sh, sw, pos_h, pos_w, 0, 0, 0])
        params = torch.tensor(rows, dtype=torch.int32).reshape(B, 8)
        return params.pin_memory() if torch.cuda.is_available() else params

    def __call__(self, rgb_u8, modal_u8, gt_u8, params, out=None):
        """rgb_u8 [B,H0,W0,3], modal_u8 [B,H0,W0] or [B,H0,W0,3], gt_u8 [B,H0,W0]: contiguous uint8 on one GPU.
        A CPU `params` is range-checked here and copied with non_blocking; a device `params` is used in place
        with no host read, which makes the call capturable into a HIP graph (the kernel clamps every index,
        whatever the values). out = (rgb, modal, label) is written in place and returned."""
        if not params.is_cuda:
            check_params(params, rgb_u8.shape[0])
            params = params.to(rgb_u8.device, non_blocking=True)
        return self._run(rgb_u8, modal_u8, gt_u8, params, self.crop_size, out)


class ValPre(_Pre):
    """The reference's ValPre: normalisation only (the same kernel with identity parameters); the outputs
    have the raw size."""

    def __init__(self, norm_mean, norm_std, modal_mean=None, modal_std=None, transform_gt=False, bgr=False):
        super().__init__(norm_mean, norm_std, modal_mean, modal_std, transform_gt, bgr)
        self._params = {}

    def __call__(self, rgb_u8, modal_u8, gt_u8, out=None):
        B, H0, W0 = rgb_u8.shape[:3]
        key = (B, H0, W0, rgb_u8.device)
        if key not in self._params:  # built once per shape, so later calls read nothing from the host
            self._params[key] = torch.tensor([[0, H0, W0, 0, 0, 0, 0, 0]] * B, dtype=torch.int32, device=rgb_u8.device)
        return self._run(rgb_u8, modal_u8, gt_u8, self._params[key], (H0, W0), out)
