"""Host binding of the plan-level C ABI (include/ctrlv_hip.h: ctrlv_plan_*, ctrlv_unet_forward,
ctrlv_controlnet_forward): one ctypes call = one model forward, walked in C++ (csrc/plan.hip).

This is what `UNetSpatioTemporalConditionModel.forward` / `ControlNetModel.forward` run by default; the per-op Python
executor in models/blocks.py issues the same kernels with the same descriptors (bit-identical results) and is kept for
per-block tests, the error-growth trace and the per-kernel timing of bench.py.
"""
import collections
import ctypes

import torch

from . import _lib
from ._lib import ModelConfig, TensorDesc, check

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _tup(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


def config_struct(kind, cfg, time_context_order="sb"):
    """diffusers-style model config (dict / FrozenConfig) -> ctrlv_model_config."""
    down = tuple(cfg["down_block_types"])
    n = len(down)
    if n > _lib.CTRLV_MAX_BLOCKS:
        raise ValueError(f"at most {_lib.CTRLV_MAX_BLOCKS} blocks are supported, got {n}")
    c = ModelConfig()
    c.kind = 0 if kind == "unet" else 1
    c.in_channels = cfg["in_channels"]
    c.out_channels = cfg.get("out_channels", 4)
    c.n_blocks = n
    boc = tuple(cfg["block_out_channels"])
    heads = _tup(cfg["num_attention_heads"], n)
    layers = _tup(cfg["layers_per_block"], n)
    cross = _tup(cfg["cross_attention_dim"], n)
    if len(set(cross)) != 1:
        raise ValueError("ctrlv_amd supports one cross_attention_dim for all blocks (the SVD configuration)")
    up = tuple(cfg.get("up_block_types", ()))
    for i in range(n):
        c.block_out_channels[i] = boc[i]
        c.down_cross_attn[i] = 1 if down[i] == "CrossAttnDownBlockSpatioTemporal" else 0
        c.up_cross_attn[i] = 1 if (kind == "unet" and up[i] == "CrossAttnUpBlockSpatioTemporal") else 0
        c.layers_per_block[i] = layers[i]
        c.num_attention_heads[i] = heads[i]
    c.cross_attention_dim = cross[0]
    c.addition_time_embed_dim = cfg["addition_time_embed_dim"]
    c.projection_class_embeddings_input_dim = cfg["projection_class_embeddings_input_dim"]
    c.num_frames = cfg.get("num_frames", 25) or 25
    c.time_context_order = 0 if time_context_order == "sb" else 1
    return c


def _tensor_descs(state_dict, floating_only):
    """(TensorDesc array, the tensors it points into) of a state dict: every tensor, or the floating-point ones only.
    Keep the second value alive until the library has read the array."""
    items = [(k, v.detach()) for k, v in state_dict.items()
             if torch.is_tensor(v) and (v.is_floating_point() or not floating_only)]
    keep = []
    arr = (TensorDesc * len(items))()
    for i, (k, v) in enumerate(items):
        if v.dtype not in _DT:
            v = v.float()
        v = v.contiguous()
        keep.append(v)
        arr[i].name = k.encode()
        arr[i].data = v.data_ptr()
        arr[i].dtype = _DT[v.dtype]
        arr[i].on_device = 1 if v.is_cuda else 0
        arr[i].numel = v.numel()
    return arr, keep


class _Handle:
    """What the plan objects share: the library and the C handle with its destroy symbol, the hand-over of a state dict, the
    current stream, the "a size query answered 0" idiom and one workspace per stream."""
    _destroy = None          # name of the library's destroy call for this kind of handle

    def _open(self, device, dtype):
        self.device = torch.device(device)
        self.dtype = dtype
        self._lib = _lib.load(dtype)
        self._h = ctypes.c_void_p()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                getattr(self._lib, self._destroy)(h)
            except Exception:       # noqa: BLE001  (interpreter shutdown)
                pass

    def _load(self, symbol, state_dict, floating_only):
        """Hand every (floating-point) parameter to the library by its key; packing happens on the device in C++."""
        arr, keep = _tensor_descs(state_dict, floating_only)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)          # parameters may still be in flight on torch's streams
        check(getattr(self._lib, symbol)(self._h, arr, len(arr)), symbol)
        del keep

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _nonzero(self, n, symbol):
        """The answer of a size query; 0 means refused: raise the library's message."""
        if n == 0:
            check(-2, symbol, lib=self._lib)
        return n

    def _stream_workspace(self, need):
        """A uint8 tensor of at least `need` bytes, one per stream (self._ws: stream -> tensor)."""
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws


class Plan(_Handle):
    """Owns one `ctrlv_plan` (module graph + packed weights in library-owned device memory)."""
    _destroy = "ctrlv_plan_destroy"

    def __init__(self, kind, config, device, time_context_order="sb", dtype=torch.bfloat16):
        """dtype: the ELEMENT type of the plan's activations and packed weights -- torch.bfloat16 (libctrlv_hip.so) or
        torch.float16 (libctrlv_hip_f16.so)."""
        self.kind = kind
        self._open(device, dtype)
        self._cfg = config_struct(kind, config, time_context_order)
        check(self._lib.ctrlv_plan_create(ctypes.byref(self._cfg), self.device.index or 0, ctypes.byref(self._h)),
              "ctrlv_plan_create")
        self.trunk_mode = "same"
        self.ff_mode = "same"
        self._ws = {}            # lane -> uint8 workspace tensor
        self._ws_bytes = {}      # (B, F, H, W) -> bytes
        self.n_down = self._lib.ctrlv_plan_num_down_residuals(self._h)

    def load_state_dict(self, state_dict):
        """Hand every parameter to the library by its diffusers key; packing happens on the device in C++."""
        self._load("ctrlv_plan_load_weights", state_dict, floating_only=False)

    def profile(self, enable=True):
        """Bracket every kernel the plan issues with HIP events (eager forwards only; not under graph capture)."""
        check(self._lib.ctrlv_plan_profile(self._h, 1 if enable else 0), "ctrlv_plan_profile")

    def profile_read(self):
        """[(family, ms, flops, bytes, (M, N, K, flags))] of the launches since profile(True), in launch order."""
        n = self._lib.ctrlv_plan_profile_read(self._h, None, 0)
        if n <= 0:
            return []
        arr = (_lib.ProfileRecord * n)()
        m = self._lib.ctrlv_plan_profile_read(self._h, arr, n)
        if m < 0:
            check(m, "ctrlv_plan_profile_read")
        return [(_lib.FAMILIES[r.family], r.ms, r.flops, r.bytes, (r.M, r.N, r.K, r.flags)) for r in arr[:m]]

    def set_trunk_mode(self, mode):
        """Storage of the residual trunk: "same" (one element per value) or "fp16x2" (split: an fp16 hi plane + a one-byte
        e5m2 lo plane, ~15 significant bits in 3 bytes; fp16 plans only; the name is the API's since round 5) -- ctrlv_plan_set_trunk_mode."""
        if mode not in ("same", "fp16x2"):
            raise ValueError(f'trunk_dtype must be "same" or "fp16x2", got {mode!r}')
        check(self._lib.ctrlv_plan_set_trunk_mode(self._h, 1 if mode == "fp16x2" else 0), "ctrlv_plan_set_trunk_mode")
        self._ws_bytes.clear()          # the workspace grows with the lo planes
        self.trunk_mode = mode

    def set_ff_precision(self, mode):
        """Precision of the transformer feed-forwards: "same" (the element type) or "f8" (e4m3 operands on the block-scaled
        MFMA wherever ctrlv_gemm_f8_serves accepts the layer; opt-in throughput mode) -- ctrlv_plan_set_ff_precision."""
        if mode not in ("same", "f8"):
            raise ValueError(f'ff_dtype must be "same" or "f8", got {mode!r}')
        check(self._lib.ctrlv_plan_set_ff_precision(self._h, 1 if mode == "f8" else 0), "ctrlv_plan_set_ff_precision")
        self._ws_bytes.clear()          # the workspace grows with the codes and scales
        self.ff_mode = mode

    def set_time_context_order(self, order):
        check(self._lib.ctrlv_plan_set_time_context_order(self._h, 0 if order == "sb" else 1),
              "ctrlv_plan_set_time_context_order")

    def workspace_bytes(self, B, F, H, W):
        key = (B, F, H, W)
        if key not in self._ws_bytes:
            self._ws_bytes[key] = self._nonzero(self._lib.ctrlv_plan_workspace_bytes(self._h, B, F, H, W),
                                                "ctrlv_plan_workspace_bytes")
        return self._ws_bytes[key]

    def workspace(self, B, F, H, W, lane=0):
        need = self.workspace_bytes(B, F, H, W)
        ws = self._ws.get(lane)
        if ws is None or ws.numel() < need or ws.device != self.device:
            ws = self._ws[lane] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def residual_shape(self, i, B, F, H, W):
        rows, ch = ctypes.c_int64(), ctypes.c_int32()
        check(self._lib.ctrlv_plan_residual_shape(self._h, i, B, F, H, W, ctypes.byref(rows), ctypes.byref(ch)),
              "ctrlv_plan_residual_shape")
        return rows.value, ch.value

    def unet_forward(self, sample, t32, ehs, ids32, down_rows, mid_rows, out, residual_event=None, lane=0):
        B, F, _, H, W = sample.shape
        ws = self.workspace(B, F, H, W, lane)
        down = None
        if down_rows is not None:
            down = (ctypes.c_void_p * len(down_rows))(*[r.data_ptr() for r in down_rows])
        ev = ctypes.c_void_p(residual_event.cuda_event) if residual_event is not None else None
        check(self._lib.ctrlv_unet_forward(
            self._h, sample.data_ptr(), _DT[sample.dtype], t32.data_ptr(), t32.numel(), ehs.data_ptr(),
            ids32.data_ptr(), ids32.shape[1], down, mid_rows.data_ptr() if mid_rows is not None else None, ev,
            out.data_ptr(), B, F, H, W, ws.data_ptr(), ws.numel(), self._stream()), "ctrlv_unet_forward")
        return out

    def unet_encoder_forward(self, sample, t32, ehs, ids32, out_taps, out_mid, lane=0):
        """Down + mid path only: writes the skip tensors / mid output into caller-owned row tensors (training step)."""
        B, F, _, H, W = sample.shape
        ws = self.workspace(B, F, H, W, lane)
        outs = (ctypes.c_void_p * len(out_taps))(*[r.data_ptr() for r in out_taps])
        check(self._lib.ctrlv_unet_encoder_forward(
            self._h, sample.data_ptr(), _DT[sample.dtype], t32.data_ptr(), t32.numel(), ehs.data_ptr(),
            ids32.data_ptr(), ids32.shape[1], outs, out_mid.data_ptr(), B, F, H, W, ws.data_ptr(), ws.numel(),
            self._stream()), "ctrlv_unet_encoder_forward")

    def controlnet_forward(self, sample, control, t32, ehs, ids32, scale, out_down, out_mid, lane=0):
        B, F, _, H, W = sample.shape
        ws = self.workspace(B, F, H, W, lane)
        outs = (ctypes.c_void_p * len(out_down))(*[r.data_ptr() for r in out_down])
        check(self._lib.ctrlv_controlnet_forward(
            self._h, sample.data_ptr(), control.data_ptr(), _DT[sample.dtype], t32.data_ptr(), t32.numel(),
            ehs.data_ptr(), ids32.data_ptr(), ids32.shape[1], float(scale), outs, out_mid.data_ptr(), B, F, H, W,
            ws.data_ptr(), ws.numel(), self._stream()), "ctrlv_controlnet_forward")


CLIP_ACTS = {"gelu": 0, "quick_gelu": 1}


class ClipPlan(_Handle):
    """Owns one `ctrlv_clip_plan`: the CLIP vision tower (transformers' CLIPVisionModelWithProjection) as one C call --
    create, `load_state_dict` (transformers' keys), workspace, `forward` (include/ctrlv_hip.h)."""
    _destroy = "ctrlv_clip_plan_destroy"

    def __init__(self, config, device, dtype=torch.bfloat16):
        """config: transformers' CLIPVisionConfig fields (a dict); dtype: the element type, as for `Plan`."""
        self._open(device, dtype)
        act = config["hidden_act"]
        if act not in CLIP_ACTS:
            raise ValueError(f"ClipPlan: hidden_act {act!r} (gelu or quick_gelu)")
        c = self._cfg = _lib.ClipConfig()
        for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
                  "projection_dim"):
            setattr(c, k, int(config[k]))
        c.hidden_act = CLIP_ACTS[act]
        c.layer_norm_eps = float(config.get("layer_norm_eps", 1e-5))
        check(self._lib.ctrlv_clip_plan_create(ctypes.byref(c), self.device.index or 0, ctypes.byref(self._h)),
              "ctrlv_clip_plan_create")
        self.tokens = (c.image_size // c.patch_size) ** 2 + 1
        self._ws = {}            # stream -> uint8 workspace tensor

    def load_state_dict(self, state_dict):
        """Hand every parameter to the library by its transformers key; packing happens on the device in C++."""
        self._load("ctrlv_clip_plan_load_weights", state_dict, floating_only=True)

    def workspace_bytes(self, n_img):
        return self._nonzero(self._lib.ctrlv_clip_plan_workspace_bytes(self._h, n_img), "ctrlv_clip_plan_workspace_bytes")

    def workspace(self, n_img):
        return self._stream_workspace(self.workspace_bytes(n_img))

    def forward(self, pixel_values, return_hidden=False, workspace=None):
        """image_embeds [n, projection_dim] (and last_hidden_state [n, tokens, hidden]) in the plan's element type, enqueued on
        torch's current stream."""
        if pixel_values.dim() != 4 or pixel_values.dtype not in _DT or not pixel_values.is_cuda:
            raise ValueError("ClipPlan.forward: pixel_values must be a (n, 3, H, W) fp32 / fp16 / bf16 tensor on the HIP device")
        if pixel_values.device != self.device and (pixel_values.device.index or 0) != (self.device.index or 0):
            raise ValueError(f"ClipPlan.forward: pixel_values on {pixel_values.device}, the plan's weights on {self.device}")
        c = self._cfg
        if tuple(pixel_values.shape[1:]) != (3, c.image_size, c.image_size):
            raise ValueError(f"ClipPlan.forward: pixel_values {tuple(pixel_values.shape)}, the plan is for 3 x {c.image_size}^2")
        px = pixel_values.contiguous()
        n = px.shape[0]
        ws = self.workspace(n) if workspace is None else workspace
        embeds = torch.empty(n, c.projection_dim, dtype=self.dtype, device=self.device)
        hidden = torch.empty(n, self.tokens, c.hidden_size, dtype=self.dtype, device=self.device) if return_hidden else None
        check(self._lib.ctrlv_clip_forward(self._h, px.data_ptr(), _DT[px.dtype], n, embeds.data_ptr(),
                                           hidden.data_ptr() if return_hidden else None, ws.data_ptr(), ws.numel(),
                                           self._stream()), "ctrlv_clip_forward")
        return (embeds, hidden) if return_hidden else embeds


class LpipsPlan(_Handle):
    """Owns one `ctrlv_lpips_plan`: LPIPS (AlexNet, v0.1) of frame pairs as one C call on split 16-bit operands
    (include/ctrlv_hip.h "LPIPS of generated frames") -- create, load the weights, workspace, `frames`."""
    _destroy = "ctrlv_lpips_plan_destroy"
    _SRC = {torch.float32: 0, torch.uint8: 3}

    def __init__(self, weights, device, dtype=torch.bfloat16):
        """weights: a models.lpips_alex.LpipsAlexWeights, or a state dict with its names; dtype: the element type the operands
        are split in, as for `Plan`."""
        self._open(device, dtype)
        check(self._lib.ctrlv_lpips_plan_create(self.device.index or 0, ctypes.byref(self._h)), "ctrlv_lpips_plan_create")
        self._ws = {}            # stream -> uint8 workspace tensor
        self.load_state_dict(weights.state_dict() if hasattr(weights, "state_dict") else weights)

    def load_state_dict(self, state_dict):
        self._load("ctrlv_lpips_plan_load_weights", state_dict, floating_only=True)

    def workspace_bytes(self, H, W, frames_per_chunk=1):
        return self._nonzero(self._lib.ctrlv_lpips_ws_bytes(self._h, int(H), int(W), int(frames_per_chunk)), "ctrlv_lpips_ws_bytes")

    def frames(self, gt, gen, workspace=None, frames_per_chunk=8):
        """gt, gen: (n, F, 3, H, W) uint8, or fp32 in [-1, 1], on the plan's device -> float64 (n, F) on the device: the LPIPS of
        every frame pair.  workspace: a uint8 tensor (256-byte aligned) to use; else one of the plan's, sized for
        frames_per_chunk frame pairs at a time.  A frame's bits depend on neither.  No host sync."""
        fn = "LpipsPlan.frames"
        if gt.dim() != 5 or gt.shape[2] != 3 or gt.dtype not in self._SRC or not gt.is_cuda:
            raise ValueError(f"{fn}: gt must be (n, F, 3, H, W) uint8 or fp32 on the HIP device")
        if tuple(gen.shape) != tuple(gt.shape) or gen.dtype != gt.dtype or gen.device != gt.device:
            raise ValueError(f"{fn}: gen must be {gt.dtype} {tuple(gt.shape)} on {gt.device}, got {gen.dtype} {tuple(gen.shape)} on "
                             f"{gen.device}")
        if (gt.device.index or 0) != (self.device.index or 0):
            raise ValueError(f"{fn}: frames on {gt.device}, the plan's weights on {self.device}")
        gt, gen = gt.contiguous(), gen.contiguous()
        n, F, _, H, W = gt.shape
        if workspace is None:
            workspace = self._stream_workspace(self.workspace_bytes(H, W, max(1, min(int(frames_per_chunk), n * F))))
        out = torch.empty(n, F, dtype=torch.float64, device=gt.device)
        check(self._lib.ctrlv_lpips_frames(self._h, gt.data_ptr(), gen.data_ptr(), self._SRC[gt.dtype], n, F, H, W, out.data_ptr(),
                                           workspace.data_ptr(), workspace.numel() * workspace.element_size(), self._stream()),
              "ctrlv_lpips_frames")
        return out


class VaePlan(_Handle):
    """Owns one `ctrlv_vae_plan`: the SVD VAE (AutoencoderKLTemporalDecoder) as one C call each way -- create,
    `load_state_dict` (diffusers keys: encoder.*, decoder.*, quant_conv.*), workspace, `encode` / `decode`
    (include/ctrlv_hip.h).  The plan runs in bf16 elements: the Python layer routes the VAE to libctrlv_hip.so."""
    _destroy = "ctrlv_vae_plan_destroy"

    def __init__(self, config, device, offset_limit_bytes=0, dtype=torch.bfloat16):
        """config: the fields of AutoencoderKLTemporalDecoder's config (a dict or its config object).  dtype: the element type;
        torch.float16 selects libctrlv_hip_f16.so's build of the same walk (what a PipelinePlan of fp16 models borrows)."""
        get = config.get if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
        self._open(device, dtype)
        c = self._cfg = _lib.VaeConfig()
        boc = tuple(get("block_out_channels"))
        if len(boc) > _lib.CTRLV_MAX_BLOCKS:
            raise ValueError(f"VaePlan: {len(boc)} blocks, at most {_lib.CTRLV_MAX_BLOCKS}")
        c.in_channels, c.out_channels = int(get("in_channels")), int(get("out_channels"))
        c.latent_channels, c.layers_per_block, c.n_blocks = int(get("latent_channels")), int(get("layers_per_block")), len(boc)
        for i, ch in enumerate(boc):
            c.block_out_channels[i] = int(ch)
        c.scaling_factor = float(get("scaling_factor", 0.18215))
        c.offset_limit_bytes = int(offset_limit_bytes)
        check(self._lib.ctrlv_vae_plan_create(ctypes.byref(c), self.device.index or 0, ctypes.byref(self._h)),
              "ctrlv_vae_plan_create")
        self._ws = {}            # stream -> uint8 workspace tensor

    def load_state_dict(self, state_dict):
        """Hand every parameter to the library by its diffusers key; packing happens on the device in C++."""
        self._load("ctrlv_vae_plan_load_weights", state_dict, floating_only=True)

    def workspace_bytes(self, what, n, num_frames, H, W):
        """what: "encode" (n images of H x W pixels) or "decode" (n latent frames of H x W latent pixels, clips of num_frames)."""
        return self._nonzero(self._lib.ctrlv_vae_plan_workspace_bytes(self._h, {"encode": 0, "decode": 1}[what], n, num_frames, H, W),
                             "ctrlv_vae_plan_workspace_bytes")

    def workspace(self, what, n, num_frames, H, W):
        return self._stream_workspace(self.workspace_bytes(what, n, num_frames, H, W))

    def _check(self, t, what):
        if t.dim() != 4 or t.dtype not in _DT or not t.is_cuda:
            raise ValueError(f"VaePlan.{what}: a 4-D fp32 / fp16 / bf16 tensor on the HIP device")
        if (t.device.index or 0) != (self.device.index or 0):
            raise ValueError(f"VaePlan.{what}: input on {t.device}, the plan's weights on {self.device}")

    def encode(self, x, noise=None, scale=1.0, moments=True, workspace=None, out_dtype=None):
        """x (n, 3, H, W) in [-1, 1] -> (latents, moments): latents (n, L, H/8, W/8) = scale * (mean + std * noise) -- noise
        fp32 (n, L, H/8, W/8), None = the distribution's mode --, moments (n, 2 L, H/8, W/8) after quant_conv (or None).  Both
        in out_dtype (default x.dtype), enqueued on torch's current stream."""
        self._check(x, "encode")
        x = x.contiguous()
        n, _, H, W = x.shape
        L = self._cfg.latent_channels
        ws = self.workspace("encode", n, 1, H, W) if workspace is None else workspace
        out_dtype = x.dtype if out_dtype is None else out_dtype
        if out_dtype not in _DT:
            raise ValueError(f"VaePlan.encode: out_dtype {out_dtype} (fp32, fp16 or bf16)")
        lat = torch.empty(n, L, H // 8, W // 8, dtype=out_dtype, device=x.device)
        mom = torch.empty(n, 2 * L, H // 8, W // 8, dtype=out_dtype, device=x.device) if moments else None
        if noise is not None:
            noise = noise.to(device=x.device, dtype=torch.float32).contiguous()
            if noise.shape != lat.shape:
                raise ValueError(f"VaePlan.encode: noise {tuple(noise.shape)} must be {tuple(lat.shape)}")
        check(self._lib.ctrlv_vae_encode(self._h, x.data_ptr(), _DT[x.dtype], n, H, W,
                                         noise.data_ptr() if noise is not None else None, float(scale), lat.data_ptr(),
                                         mom.data_ptr() if moments else None, _DT[out_dtype], ws.data_ptr(), ws.numel(),
                                         self._stream()), "ctrlv_vae_encode")
        return lat, mom

    def decode(self, z, num_frames, workspace=None, out=None):
        """z (n, L, h, w) latents already divided by the scaling factor -> frames (n, 3, 8 h, 8 w) in z.dtype."""
        self._check(z, "decode")
        z = z.contiguous()
        n, _, h, w = z.shape
        ws = self.workspace("decode", n, num_frames, h, w) if workspace is None else workspace
        if out is None:
            out = torch.empty(n, self._cfg.out_channels, 8 * h, 8 * w, dtype=z.dtype, device=z.device)
        check(self._lib.ctrlv_vae_decode(self._h, z.data_ptr(), _DT[z.dtype], n, num_frames, h, w, out.data_ptr(),
                                         _DT[out.dtype], ws.data_ptr(), ws.numel(), self._stream()), "ctrlv_vae_decode")
        return out


def euler_schedule(num_steps, sigma_min=0.0, sigma_max=0.0):
    """EulerDiscreteScheduler.set_timesteps' tables from the library (ctrlv_euler_schedule: host arithmetic in double, no GPU):
    (sigmas [num_steps + 1], timesteps [num_steps], init_noise_sigma) as Python floats holding the fp32 values.  Both bounds 0:
    SVD's 0.002 and 700."""
    n = int(num_steps)
    room = min(max(n, 1), 1024)
    sig, ts, ins = (ctypes.c_float * (room + 1))(), (ctypes.c_float * room)(), ctypes.c_double()
    check(_lib.load().ctrlv_euler_schedule(n, float(sigma_min), float(sigma_max), sig, ts, ctypes.byref(ins)),
          "ctrlv_euler_schedule")
    return list(sig), list(ts), ins.value


StageRequest = collections.namedtuple("StageRequest", "request seed_request cond out keep")
StageRequest.__doc__ = """One stage of a driver call: its `ctrlv_clip_request`, its `ctrlv_seed_request` (None without a seed), the
contiguous condition or box frames, out = (out_latents, out_frames, out_frames_u8), and in `keep` every other object the
request points into.  Hold the record until the call has been enqueued."""


class PipelinePlan(_Handle):
    """Owns one `ctrlv_pipeline`: a whole clip as one C call (include/ctrlv_hip.h: ctrlv_pipeline_generate) on four borrowed
    plans of ONE library -- `Plan("unet")`, `Plan("controlnet")` or None, `VaePlan`, `ClipPlan`.  The object keeps them alive."""
    _destroy = "ctrlv_pipeline_destroy"

    def __init__(self, unet_plan, controlnet_plan, vae_plan, clip_plan):
        self.unet, self.controlnet, self.vae, self.clip = unet_plan, controlnet_plan, vae_plan, clip_plan
        self.dtype = unet_plan.dtype
        self.device = unet_plan.device
        self._lib = unet_plan._lib
        for q in (controlnet_plan, vae_plan, clip_plan):
            if q is not None and q._lib is not self._lib:
                raise ValueError("PipelinePlan: the four plans must come from one library (one element type)")
        self._h = ctypes.c_void_p()
        check(self._lib.ctrlv_pipeline_create(unet_plan._h, controlnet_plan._h if controlnet_plan is not None else None,
                                              vae_plan._h, clip_plan._h, self.device.index or 0, ctypes.byref(self._h)),
              "ctrlv_pipeline_create")
        self._ws = None

    def set_overlap(self, on):
        check(self._lib.ctrlv_pipeline_set_overlap(self._h, 1 if on else 0), "ctrlv_pipeline_set_overlap")

    def request(self, image_u8, latents, sigmas, timesteps, *, cond=None, aug_noise=None, noise_aug_strength=0.02, fps=7,
                motion_bucket_id=127, min_guidance=1.0, max_guidance=3.0, conditioning_scale=1.0, decode_chunk=None,
                clip_mean=None, clip_std=None, out_latents=None, out_frames=None, out_frames_u8=None):
        """The `ctrlv_clip_request` of a call plus the objects its pointers refer to (keep the pair together)."""
        n, H, W, _ = image_u8.shape
        F = latents.shape[1]
        sig = (ctypes.c_float * len(sigmas))(*[float(v) for v in sigmas])
        ts = (ctypes.c_float * len(timesteps))(*[float(v) for v in timesteps])
        r = _lib.ClipRequest()
        r.n_clips, r.num_frames, r.height, r.width = n, F, H, W
        r.image_u8 = image_u8.data_ptr()
        r.num_steps = len(timesteps)
        r.latents = latents.data_ptr()
        r.sigmas, r.timesteps = sig, ts
        self._request_fields(r, cond, aug_noise, noise_aug_strength, fps, motion_bucket_id, min_guidance, max_guidance,
                             conditioning_scale, decode_chunk, clip_mean, clip_std, out_latents, out_frames, out_frames_u8)
        return r, (sig, ts, image_u8, latents, cond, aug_noise, out_latents, out_frames, out_frames_u8)

    @staticmethod
    def _request_fields(r, cond=None, aug_noise=None, noise_aug_strength=0.02, fps=7, motion_bucket_id=127, min_guidance=1.0,
                        max_guidance=3.0, conditioning_scale=1.0, decode_chunk=None, clip_mean=None, clip_std=None,
                        out_latents=None, out_frames=None, out_frames_u8=None):
        """The fields of a request beside its geometry, image, latents and schedule."""
        if cond is not None:
            r.cond, r.cond_channels, r.cond_dtype = cond.data_ptr(), cond.shape[2], _DT[cond.dtype]
        if aug_noise is not None:
            r.aug_noise = aug_noise.data_ptr()
        r.noise_aug_strength = float(noise_aug_strength)
        r.fps, r.motion_bucket_id = int(fps), int(motion_bucket_id)
        r.min_guidance, r.max_guidance = float(min_guidance), float(max_guidance)
        r.conditioning_scale = float(conditioning_scale)
        r.decode_chunk = int(r.num_frames if decode_chunk is None else decode_chunk)
        if clip_mean is not None:
            for i in range(3):
                r.clip_mean[i], r.clip_std[i] = float(clip_mean[i]), float(clip_std[i])
        for name, t in (("out_latents", out_latents), ("out_frames", out_frames), ("out_frames_u8", out_frames_u8)):
            if t is not None:
                setattr(r, name, t.data_ptr())

    def workspace_bytes(self, request):
        return self._nonzero(self._lib.ctrlv_pipeline_workspace_bytes(self._h, ctypes.byref(request)),
                             "ctrlv_pipeline_workspace_bytes")

    def _workspace(self, need):
        if self._ws is None or self._ws.numel() < need or self._ws.device != self.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _stage_request(self, who, image_u8, *, seed=None, prepare=False, latents=None, sigmas=None, timesteps=None, num_steps=None,
                       num_frames=None, height=None, width=None, clip_index0=0, call=0, sigma_min=0.0, sigma_max=0.0, cond=None,
                       cond_name="cond", aug_noise=None, frames=True, frames_u8=True, **kw):
        """Validate the tensors of one stage, allocate its outputs and build its `StageRequest`.  `cond` is the ControlNet
        condition of generate (cond_name "cond") or the box frames of predict_boxes, which do not enter the request.  With
        `seed=`: the `ctrlv_seed_request` beside it; image_u8 (n, Hs, Ws, 3) may have ANY size -- the library resizes it to
        (height, width), default its own --, and whatever of latents / aug_noise / sigmas / timesteps is not given stays NULL for
        ctrlv_pipeline_prepare to fill from (seed, clip_index0, call); `prepare=True` runs it and swaps the filled request in."""
        dev = self.device
        for name, t in (("image_u8", image_u8), ("latents", latents), (cond_name, cond), ("aug_noise", aug_noise)):
            if t is not None and (not t.is_cuda or (t.device.index or 0) != (dev.index or 0)):
                raise ValueError(f"PipelinePlan.{who}: {name} on {t.device}, the plans' weights on {dev}")
        if image_u8.dtype != torch.uint8 or image_u8.dim() != 4 or image_u8.shape[3] != 3:
            raise ValueError(f"PipelinePlan.{who}: image_u8 must be (n, H, W, 3) uint8")
        n, Hs, Ws, _ = image_u8.shape
        H, W = int(height or Hs), int(width or Ws)
        if seed is None and (H, W) != (Hs, Ws):
            raise ValueError(f"PipelinePlan.{who}: image_u8 of another size than {H} x {W} is resized with seed= only")
        L = self.vae._cfg.latent_channels
        if latents is not None:
            if latents.dtype != torch.float32 or latents.dim() != 5:
                raise ValueError(f"PipelinePlan.{who}: latents must be fp32 (n, F, L, h, w)")
            if seed is None:
                L, num_frames = latents.shape[2], latents.shape[1]
            num_frames = latents.shape[1] if num_frames is None else num_frames
            if tuple(latents.shape) != (n, num_frames, L, H // 8, W // 8):
                what = f"a {n} x {H} x {W} image" if seed is None else f"{n} clips of {num_frames} x {H} x {W}"
                raise ValueError(f"PipelinePlan.{who}: latents {tuple(latents.shape)} do not match {what}")
            latents = latents.contiguous()
        if num_frames is None and cond is not None:
            num_frames = cond.shape[1]
        if num_frames is None:
            raise ValueError(f"PipelinePlan.{who}: num_frames is needed with a seed")
        F = int(num_frames)
        if (sigmas is None) != (timesteps is None):
            raise ValueError(f"PipelinePlan.{who}: sigmas and timesteps come together")
        if sigmas is not None:
            num_steps = len(timesteps)
        if num_steps is None:
            raise ValueError(f"PipelinePlan.{who}: num_steps is needed with a seed")
        if cond is not None:
            want = (n, F, 3, H, W) if cond.dim() == 5 and cond.shape[2] == 3 else (n, F, L, H // 8, W // 8)
            if tuple(cond.shape) != want or cond.dtype not in _DT:
                raise ValueError(f"PipelinePlan.{who}: {cond_name} {tuple(cond.shape)} must be {want} in fp32 / fp16 / bf16")
            cond = cond.contiguous()
        if aug_noise is not None:
            if aug_noise.dtype != torch.float32 or tuple(aug_noise.shape) != (n, 3, H, W):
                raise ValueError(f"PipelinePlan.{who}: aug_noise must be fp32 {(n, 3, H, W)}")
            aug_noise = aug_noise.contiguous()
        image_u8 = image_u8.contiguous()
        out = (torch.empty(n, F, L, H // 8, W // 8, dtype=torch.float32, device=dev),
               torch.empty(n * F, 3, H, W, dtype=self.dtype, device=dev) if frames else None,
               torch.empty(n, F, H, W, 3, dtype=torch.uint8, device=dev) if frames_u8 else None)
        r = _lib.ClipRequest()
        r.n_clips, r.num_frames, r.height, r.width = n, F, H, W
        r.num_steps = int(num_steps)
        sig = ts = None
        if sigmas is not None:
            sig = (ctypes.c_float * len(sigmas))(*[float(v) for v in sigmas])
            ts = (ctypes.c_float * len(timesteps))(*[float(v) for v in timesteps])
            r.sigmas, r.timesteps = sig, ts
        if latents is not None:
            r.latents = latents.data_ptr()
        self._request_fields(r, cond=cond if cond_name == "cond" else None, aug_noise=aug_noise, out_latents=out[0],
                             out_frames=out[1], out_frames_u8=out[2], **kw)
        sr = sig_host = ts_host = None
        if seed is None:
            r.image_u8 = image_u8.data_ptr()
        else:                                   # image_u8 stays NULL: the source goes through the seed request
            steps = min(max(r.num_steps, 1), 1024)
            sr = _lib.SeedRequest()
            sr.seed, sr.clip_index0, sr.call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(clip_index0), int(call)
            sr.src_image_u8, sr.src_height, sr.src_width = image_u8.data_ptr(), Hs, Ws
            sr.sigma_min, sr.sigma_max = float(sigma_min), float(sigma_max)
            sig_host, ts_host = (ctypes.c_float * (steps + 1))(), (ctypes.c_float * steps)()
            sr.sigmas_host, sr.timesteps_host = sig_host, ts_host
        st = StageRequest(r, sr, cond, out, (sig, ts, image_u8, latents, aug_noise, sig_host, ts_host))
        if prepare and sr is not None:
            filled, prep_ws = self.prepare(r, sr)
            st = st._replace(request=filled, keep=(st.keep, r, prep_ws))
        return st

    def _run(self, query, call, *args):
        """One driver call in the plan's workspace, sized by the call's own query, on torch's current stream."""
        ws = self._workspace(self._nonzero(getattr(self._lib, query)(*args), query))
        check(getattr(self._lib, call)(*args, ws.data_ptr(), ws.numel(), self._stream()), call)

    def prepare(self, request, seed_request):
        """ctrlv_pipeline_prepare: the request with its NULL fields filled -- Lanczos resize, the two draws, the schedule -- and
        the device buffer the filled request points into (fresh per call: keep it until the consuming call has finished)."""
        need = self._nonzero(self._lib.ctrlv_pipeline_prepare_bytes(self._h, ctypes.byref(request), ctypes.byref(seed_request)),
                             "ctrlv_pipeline_prepare_bytes")
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = _lib.ClipRequest()
        check(self._lib.ctrlv_pipeline_prepare(self._h, ctypes.byref(request), ctypes.byref(seed_request), ctypes.byref(out),
                                               ws.data_ptr(), ws.numel(), self._stream()), "ctrlv_pipeline_prepare")
        return out, ws

    def box_render_request(self, boxes, source_size):
        """The `ctrlv_box_render_request` of a `ctrlv_amd.boxes.BoxTable` on the plan's device; keep the table alive beside it."""
        if source_size is None:
            raise ValueError("PipelinePlan: boxes= needs source_size=(Hs, Ws), the size the coordinates refer to")
        for t in (boxes.objects, boxes.frames):
            if not t.is_cuda or (t.device.index or 0) != (self.device.index or 0) or not t.is_contiguous():
                raise ValueError(f"PipelinePlan: the box table must be dense on {self.device} (BoxTable.to(device))")
        b = _lib.BoxRenderRequest()
        b.objects, b.frames = boxes.objects.data_ptr(), boxes.frames.data_ptr()
        b.n_objects, b.n_frames = boxes.n_objects, boxes.n_frames
        b.src_height, b.src_width = int(source_size[0]), int(source_size[1])
        return b

    def _rendered(self, who, boxes, source_size, height, width):
        """The box frames of a table at the working size in the plan's element type (ops.box_frames_cond)."""
        from . import ops
        if source_size is None:
            raise ValueError(f"{who}: boxes= needs source_size=(Hs, Ws), the size the coordinates refer to")
        return ops.box_frames_cond(boxes, source_size, (height, width), dtype=self.dtype)

    def generate(self, image_u8, latents=None, sigmas=None, timesteps=None, *, cond=None, aug_noise=None, frames=True,
                 frames_u8=True, seed=None, boxes=None, source_size=None, **kw):
        """image_u8 (n, H, W, 3) uint8 at the working size; latents fp32 (n, F, L, h, w) already multiplied by
        init_noise_sigma; sigmas [steps + 1] / timesteps [steps]: the scheduler's values (host floats); cond (n, F, 3, H, W)
        pixels or (n, F, L, h, w) latents; aug_noise fp32 (n, 3, H, W) or None; the other fields of `request` by keyword.
        Everything on the plan's device, enqueued on torch's current stream.  Returns (latents fp32, frames (n F, 3, H, W) in
        the element type or None, frames_u8 (n, F, H, W, 3) or None).

        With `seed=` (ctrlv_pipeline_generate_seeded): latents, sigmas and timesteps may be omitted -- give num_steps= and
        num_frames= --, image_u8 may have any size when height= and width= are given, and what is omitted comes from the
        library: see `_stage_request` for the other keywords (clip_index0, call, sigma_min, sigma_max).

        With `boxes=` (a `ctrlv_amd.boxes.BoxTable` on the device; mutually exclusive with cond) and source_size=(Hs, Ws): the
        condition is rendered from the table by the library (ctrlv_pipeline_generate_from_boxes)."""
        if seed is None and (latents is None or sigmas is None or timesteps is None):
            raise ValueError("PipelinePlan.generate: latents, sigmas and timesteps are needed without seed=")
        if boxes is not None:
            if cond is not None:
                raise ValueError("PipelinePlan.generate: boxes and cond are mutually exclusive (the library renders the condition)")
            if seed is not None:
                raise ValueError("PipelinePlan.generate: boxes= goes with explicit latents and a schedule, not with seed=")
            st = self._stage_request("generate", image_u8, latents=latents, sigmas=sigmas, timesteps=timesteps,
                                     aug_noise=aug_noise, frames=frames, frames_u8=frames_u8, **kw)
            b = self.box_render_request(boxes, source_size)
            self._run("ctrlv_pipeline_from_boxes_workspace_bytes", "ctrlv_pipeline_generate_from_boxes", self._h,
                      ctypes.byref(st.request), ctypes.byref(b))
            return st.out
        st = self._stage_request("generate", image_u8, seed=seed, latents=latents, sigmas=sigmas, timesteps=timesteps, cond=cond,
                                 aug_noise=aug_noise, frames=frames, frames_u8=frames_u8, **kw)
        if seed is None:
            self._run("ctrlv_pipeline_workspace_bytes", "ctrlv_pipeline_generate", self._h, ctypes.byref(st.request))
        else:
            self._run("ctrlv_pipeline_seeded_workspace_bytes", "ctrlv_pipeline_generate_seeded", self._h, ctypes.byref(st.request),
                      ctypes.byref(st.seed_request))
        return st.out

    @staticmethod
    def box_condition(bbox_frames, num_cond_frames):
        """The `ctrlv_box_condition` of (n, F, 3, H, W) box pixels or (n, F, L, h, w) box latents (contiguous, fp32 / fp16 /
        bf16); keep the tensor alive beside it."""
        bc = _lib.BoxCondition()
        bc.frames, bc.channels, bc.dtype = bbox_frames.data_ptr(), bbox_frames.shape[2], _DT[bbox_frames.dtype]
        bc.num_cond_frames = int(num_cond_frames)
        return bc

    def predict_boxes(self, image_u8, latents, sigmas, timesteps, bbox_frames=None, num_cond_frames=3, *, aug_noise=None, frames=True,
                      frames_u8=True, seed=None, boxes=None, source_size=None, **kw):
        """The box predictor (ctrlv_pipeline_predict_boxes; a plan without a ControlNet): `generate` with the conditioning
        channels of frames [0, num_cond_frames) and F - 1 overwritten by bbox_frames -- (n, F, 3, H, W) pixels in [-1, 1], VAE
        encoded, or (n, F, L, h, w) latents -- and the decoded frames clamped to [-1, 1].  Same returns as `generate`; with
        `seed=`, latents / sigmas / timesteps may be None: ctrlv_pipeline_prepare fills them.  `boxes=` (a `BoxTable`) with
        source_size=(Hs, Ws) instead of bbox_frames: the frames are rendered from the table first (a trajectory frame is a frame
        record with kind 1)."""
        if boxes is not None:
            # the two-call composition: ctrlv_box_frames_cond, then the predictor on its output, on one stream
            if bbox_frames is not None:
                raise ValueError("PipelinePlan.predict_boxes: boxes and bbox_frames are mutually exclusive")
            H, W = int(kw.get("height") or image_u8.shape[1]), int(kw.get("width") or image_u8.shape[2])
            bbox_frames = self._rendered("PipelinePlan.predict_boxes", boxes, source_size, H, W)
        if bbox_frames is None:
            raise ValueError("PipelinePlan.predict_boxes: bbox_frames is None")
        st = self._stage_request("predict_boxes", image_u8, seed=seed, prepare=True, latents=latents, sigmas=sigmas,
                                 timesteps=timesteps, cond=bbox_frames, cond_name="bbox_frames", aug_noise=aug_noise, frames=frames,
                                 frames_u8=frames_u8, **kw)
        bc = self.box_condition(st.cond, num_cond_frames)
        self._run("ctrlv_pipeline_boxes_workspace_bytes", "ctrlv_pipeline_predict_boxes", self._h, ctypes.byref(st.request),
                  ctypes.byref(bc))
        return st.out

    def best_boxes_request(self, who, image_u8, bbox_frames, gt_u8, guidance, num_cond_frames, *, latents=None, aug_noise=None,
                           schedule=None, seed=None, num_steps=None, clip_index0=0, clean_threshold=50.0, pt=True, cond=True,
                           u8=True, **kw):
        """The `ctrlv_best_boxes_request` of C = len(guidance) stage-1 candidates, candidate c with the guidance ramp
        guidance[c] = (min, max), latents[c] and aug_noise[c]; the other request fields (`request`) by keyword, shared.  With
        `seed=`: what is omitted of candidate c comes from ctrlv_pipeline_prepare with call = c.  Returns (request, keep,
        (pt, cond, u8, winner, counts)): keep the three together until the call has finished."""
        if bbox_frames is None or gt_u8 is None:
            raise ValueError(f"PipelinePlan.{who}: bbox_frames / gt_u8 is None")
        C = len(guidance)
        if not 1 <= C <= 8:
            raise ValueError(f"PipelinePlan.{who}: {C} guidance pairs; the library takes 1 to 8 candidates")
        for name, seq in (("latents", latents), ("aug_noise", aug_noise)):
            if seq is not None and (isinstance(seq, torch.Tensor) or len(seq) != C):
                raise ValueError(f"PipelinePlan.{who}: {name} must be a sequence of {C} tensors, one per candidate")
        sig, ts = schedule if schedule is not None else (None, None)
        if seed is None and (latents is None or sig is None):
            raise ValueError(f"PipelinePlan.{who}: latents and schedule are needed without seed=")
        stages = [self._stage_request(who, image_u8, seed=seed, prepare=True, num_steps=num_steps, num_frames=bbox_frames.shape[1],
                                      clip_index0=clip_index0, call=c, latents=latents[c] if latents is not None else None,
                                      sigmas=sig, timesteps=ts, cond=bbox_frames, cond_name="bbox_frames",
                                      aug_noise=aug_noise[c] if aug_noise is not None else None, frames=False, frames_u8=False,
                                      **dict(kw, min_guidance=g_min, max_guidance=g_max))
                  for c, (g_min, g_max) in enumerate(guidance)]
        r0 = stages[0].request
        n, F, H, W = r0.n_clips, r0.num_frames, r0.height, r0.width
        dev = self.device
        if gt_u8.dtype != torch.uint8 or tuple(gt_u8.shape) != (n, F, 3, H, W) or not gt_u8.is_cuda or \
                (gt_u8.device.index or 0) != (dev.index or 0):
            raise ValueError(f"PipelinePlan.{who}: gt_u8 must be uint8 {(n, F, 3, H, W)} on {dev}")
        gt_u8 = gt_u8.contiguous()
        out_pt = torch.empty(n * F, 3, H, W, dtype=self.dtype, device=dev) if pt else None
        out_cond = torch.empty(n * F, 3, H, W, dtype=self.dtype, device=dev) if cond else None
        out_u8 = torch.empty(n, F, 3, H, W, dtype=torch.uint8, device=dev) if u8 else None
        counts = torch.empty(C, n, 2, 3, dtype=torch.int64, device=dev)
        winner = torch.empty(n, dtype=torch.int32, device=dev)
        arr = (_lib.ClipRequest * C)(*[st.request for st in stages])
        q = _lib.BestBoxesRequest()
        q.n_candidates, q.candidates = C, arr
        q.box_cond = self.box_condition(stages[-1].cond, num_cond_frames)
        q.gt_u8, q.clean_threshold = gt_u8.data_ptr(), float(clean_threshold)
        for name, t in (("out_pt", out_pt), ("out_cond", out_cond), ("out_u8", out_u8), ("out_counts", counts),
                        ("out_winner", winner)):
            if t is not None:
                setattr(q, name, t.data_ptr())
        return q, (arr, stages, gt_u8), (out_pt, out_cond, out_u8, winner, counts)

    def best_boxes(self, image_u8, bbox_frames, gt_u8, guidance=((1, 2), (1, 3), (2, 4), (2, 5), (3, 5)), num_cond_frames=3, *,
                   latents=None, aug_noise=None, schedule=None, seed=None, num_steps=None, clip_index0=0, **kw):
        """The reference's best-of-N loop over stage-1 candidates as one C call (ctrlv_pipeline_best_boxes; a plan without a
        ControlNet): `predict_boxes` once per guidance ramp, each result cleaned (ops.box_frames_post) and counted against
        gt_u8 (n, F, 3, H, W) uint8 (ops.mask_counts), the best one per clip chosen on the device (ops.best_candidate: largest
        all-frames IoU, a tie to the later candidate) and post-processed.  latents / aug_noise: sequences, one tensor per
        candidate; schedule: (sigmas, timesteps), shared; see `best_boxes_request` for the rest.  Nothing synchronises with the
        host.  Returns (pt, cond, u8, winner, counts): the winner's [0, 1] frames and 2 (y - 0.5) condition, (n F, 3, H, W) in
        the element type, its cleaned frames (n, F, 3, H, W) uint8, the winning candidate per clip int32 (n) and every
        candidate's counts int64 (C, n, 2, 3) (metrics.candidate_scores turns them into the logged triples)."""
        q, keep, out = self.best_boxes_request("best_boxes", image_u8, bbox_frames, gt_u8, guidance, num_cond_frames, latents=latents,
                                               aug_noise=aug_noise, schedule=schedule, seed=seed, num_steps=num_steps,
                                               clip_index0=clip_index0, **kw)
        self._run("ctrlv_pipeline_best_boxes_workspace_bytes", "ctrlv_pipeline_best_boxes", self._h, ctypes.byref(q))
        return out


def _video_stage(who, video_plan, image_u8, num_frames, video_latents, video_schedule, video_aug_noise, frames, frames_u8, video_kw,
                 seed, num_steps, clip_index0, call):
    """Stage 2 of a chain: `video_plan.generate`'s request without its cond, which the chain call supplies."""
    if seed is None and (video_latents is None or video_schedule is None):
        raise ValueError(f"{who}: video_latents and video_schedule are needed without seed=")
    sig, ts = video_schedule if video_schedule is not None else (None, None)
    return video_plan._stage_request(who, image_u8, seed=seed, prepare=True, num_steps=num_steps, num_frames=num_frames,
                                     clip_index0=clip_index0, call=call, latents=video_latents, sigmas=sig, timesteps=ts,
                                     aug_noise=video_aug_noise, frames=frames, frames_u8=frames_u8, **(video_kw or {}))


def best_boxes_to_video(boxes_plan, video_plan, image_u8, bbox_frames, gt_u8, guidance=((1, 2), (1, 3), (2, 4), (2, 5), (3, 5)),
                        num_cond_frames=3, *, box_latents=None, video_latents=None, box_schedule=None, video_schedule=None,
                        box_aug_noise=None, video_aug_noise=None, clean_threshold=50.0, box_frames_u8=True, frames=True,
                        frames_u8=True, box_kw=None, video_kw=None, seed=None, num_steps=None, clip_index0=0):
    """`boxes_plan.best_boxes` and `video_plan.generate` conditioned on the winner's frames, as one C call
    (ctrlv_pipeline_best_boxes_to_video).  box_latents / box_aug_noise: one tensor per candidate; the rest as `boxes_to_video`.
    With `seed=`: candidate c draws with call = c, stage 2 with call = C (for one candidate the convention of `boxes_to_video`);
    num_steps: one count or (stage 1, stage 2).  Returns what `boxes_to_video` returns plus (winner int32 (n), counts int64
    (C, n, 2, 3))."""
    if boxes_plan._lib is not video_plan._lib:
        raise ValueError("best_boxes_to_video: the two pipeline plans must come from one library (one element type)")
    steps = tuple(num_steps) if isinstance(num_steps, (tuple, list)) else (num_steps, num_steps)
    qb, keep_b, (_, _, clean, winner, counts) = boxes_plan.best_boxes_request(
        "best_boxes_to_video", image_u8, bbox_frames, gt_u8, guidance, num_cond_frames, latents=box_latents, aug_noise=box_aug_noise,
        schedule=box_schedule, seed=seed, num_steps=steps[0], clip_index0=clip_index0, clean_threshold=clean_threshold, pt=False,
        cond=False, u8=box_frames_u8, **(box_kw or {}))
    sv = _video_stage("best_boxes_to_video", video_plan, image_u8, bbox_frames.shape[1], video_latents, video_schedule,
                      video_aug_noise, frames, frames_u8, video_kw, seed, steps[1], clip_index0, len(guidance))
    q = _lib.BestChainRequest()
    q.boxes, q.video = qb, sv.request
    video_plan._run("ctrlv_pipeline_best_chain_workspace_bytes", "ctrlv_pipeline_best_boxes_to_video", boxes_plan._h, video_plan._h,
                    ctypes.byref(q))
    return sv.out + (clean, winner, counts)


def boxes_to_video(boxes_plan, video_plan, image_u8, box_latents, video_latents, box_schedule, video_schedule, bbox_frames,
                   num_cond_frames=3, *, box_aug_noise=None, video_aug_noise=None, clean_threshold=50.0, box_frames_u8=True,
                   frames=True, frames_u8=True, box_kw=None, video_kw=None, seed=None, num_steps=None, clip_index0=0):
    """The chain as one C call (ctrlv_pipeline_boxes_to_video): `boxes_plan.predict_boxes`, `ops.box_frames_post`, then
    `video_plan.generate` conditioned on the predicted box frames.  box_schedule / video_schedule: (sigmas, timesteps) of the
    two stages; box_kw / video_kw: the other request fields of each stage (see PipelinePlan.request).  Returns (video latents
    fp32, video frames or None, video frames_u8 or None, cleaned box frames (n, F, 3, H, W) uint8 or None).

    With `seed=`: the latents and schedules may be None (num_steps: one count or one per stage; image_u8 of any size with
    height / width in box_kw and video_kw); each stage's request is filled by ctrlv_pipeline_prepare, stage 1 drawing with
    call = 0 and stage 2 with call = 1, and the chain call itself is the same."""
    if boxes_plan._lib is not video_plan._lib:
        raise ValueError("boxes_to_video: the two pipeline plans must come from one library (one element type)")
    if bbox_frames is None:
        raise ValueError("boxes_to_video: bbox_frames is None")
    steps = tuple(num_steps) if isinstance(num_steps, (tuple, list)) else (num_steps, num_steps)
    sig, ts = box_schedule if box_schedule is not None else (None, None)
    sb = boxes_plan._stage_request("boxes_to_video", image_u8, seed=seed, prepare=True, num_steps=steps[0],
                                   num_frames=bbox_frames.shape[1], clip_index0=clip_index0, call=0, latents=box_latents, sigmas=sig,
                                   timesteps=ts, cond=bbox_frames, cond_name="bbox_frames", aug_noise=box_aug_noise, frames=False,
                                   frames_u8=False, **(box_kw or {}))
    sv = _video_stage("boxes_to_video", video_plan, image_u8, bbox_frames.shape[1], video_latents, video_schedule, video_aug_noise,
                      frames, frames_u8, video_kw, seed, steps[1], clip_index0, 1)
    rb = sb.request
    clean = torch.empty(rb.n_clips, rb.num_frames, 3, rb.height, rb.width, dtype=torch.uint8, device=video_plan.device) \
        if box_frames_u8 else None
    q = _lib.TwoStageRequest()
    q.boxes, q.video, q.box_cond = rb, sv.request, boxes_plan.box_condition(sb.cond, num_cond_frames)
    q.out_box_frames_u8 = clean.data_ptr() if clean is not None else None
    q.clean_threshold = float(clean_threshold)
    video_plan._run("ctrlv_pipeline_chain_workspace_bytes", "ctrlv_pipeline_boxes_to_video", boxes_plan._h, video_plan._h,
                    ctypes.byref(q))
    return sv.out + (clean,)


TRAIN_MODES = {"controlnet": 0, "unet": 1, "boxes": 2}


class TrainBatchPlan:
    """A training batch as one C call (include/ctrlv_hip.h: ctrlv_train_batch_prepare) on a borrowed `VaePlan` and `ClipPlan`
    of ONE library: pixels plus (seed, step, clip index) in, what `train_step` / `unet_train_step` read out.  The object keeps
    the plans alive and holds the scheduler's two tables on the device."""

    def __init__(self, vae_plan, clip_plan, sigma_table=None, timestep_table=None):
        """sigma_table / timestep_table: fp32 [T]; default `EulerDiscreteScheduler().sigmas[:-1]` and `.timesteps` as __init__
        builds them (the 1000 training entries: the lookup is the reference's get_sigmas)."""
        if vae_plan._lib is not clip_plan._lib:
            raise ValueError("TrainBatchPlan: the two plans must come from one library (one element type)")
        self.vae, self.clip = vae_plan, clip_plan
        self.dtype, self.device, self._lib = vae_plan.dtype, vae_plan.device, vae_plan._lib
        if (sigma_table is None) != (timestep_table is None):
            raise ValueError("TrainBatchPlan: sigma_table and timestep_table come together")
        if sigma_table is None:
            from .schedulers import EulerDiscreteScheduler
            sched = EulerDiscreteScheduler()
            sigma_table, timestep_table = sched.sigmas[:-1], sched.timesteps
        self.sigma_table = sigma_table.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.timestep_table = timestep_table.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if self.sigma_table.dim() != 1 or self.sigma_table.shape != self.timestep_table.shape:
            raise ValueError("TrainBatchPlan: the tables must be one-dimensional and of one length")
        self._ws = None

    @staticmethod
    def _mode(mode):
        if isinstance(mode, str) and mode not in TRAIN_MODES:
            raise ValueError(f"TrainBatchPlan: mode {mode!r} (one of {', '.join(TRAIN_MODES)}, or the library's code 0 .. 2)")
        return TRAIN_MODES[mode] if isinstance(mode, str) else int(mode)

    def request(self, clips, box_frames, out, *, mode, seed, step, num_cond_frames=0, dropout_prob=None, scaling_factor=0.0,
                clip_mean=None, clip_std=None):
        """The `ctrlv_train_batch_request` of a call; `out`: name -> output tensor.  Keep the tensors alive beside it."""
        n, F, _, H, W = clips.shape
        r = _lib.TrainBatchRequest()
        r.n_clips, r.num_frames, r.height, r.width = n, F, H, W
        r.clips, r.clips_dtype = clips.data_ptr(), _DT[clips.dtype]
        if box_frames is not None:
            r.box_frames, r.box_dtype = box_frames.data_ptr(), _DT[box_frames.dtype]
        r.mode = self._mode(mode)
        r.num_cond_frames = int(num_cond_frames)
        r.dropout_prob = -1.0 if dropout_prob is None else float(dropout_prob)
        r.seed, r.clip_index0, r.call = seed.seed, seed.clip_index0, int(step) & 0xFFFFFFFF
        r.sigma_table, r.timestep_table = self.sigma_table.data_ptr(), self.timestep_table.data_ptr()
        r.table_size = self.sigma_table.numel()
        r.scaling_factor = float(scaling_factor)
        if clip_mean is not None:
            for i in range(3):
                r.clip_mean[i], r.clip_std[i] = float(clip_mean[i]), float(clip_std[i])
        for name, t in out.items():
            if name == "sample":
                r.sample_dtype = _DT[t.dtype]
            setattr(r, name, t.data_ptr())
        return r

    def workspace_bytes(self, request):
        n = self._lib.ctrlv_train_batch_workspace_bytes(self.vae._h, self.clip._h, ctypes.byref(request))
        if n == 0:
            check(-2, "ctrlv_train_batch_workspace_bytes", lib=self._lib)
        return n

    def prepare(self, clips, box_frames=None, *, mode, seed, step, num_cond_frames=0, dropout_prob=None, scaling_factor=0.0,
                clip_mean=None, clip_std=None, sample_dtype=None, return_noise=False, boxes=None, source_size=None):
        """clips / box_frames (n, F, 3, H, W) pixels in [-1, 1] (fp32, fp16 or bf16) on the plans' device; mode "controlnet"
        (box_frames become control_cond), "unet" (no box_frames) or "boxes" (the box predictor: box_frames are the target, frames
        [0, num_cond_frames) and F - 1 condition on them); seed: a `DeviceSeed`; step: the optimisation step.  Returns a dict of
        device tensors: target_latents, noisy_latents (fp32 (n, F, L, h, w)), sample ((n, F, 2 L, h, w) of sample_dtype, default
        the plans' element type), control_cond (fp32, mode "controlnet"), encoder_hidden_states ((n, 1, D) elements), sigmas,
        timesteps, random_p (fp32 (n)), indices (int32 (n)) and, with return_noise, noise.  Clip i's values depend on (seed.seed,
        seed.clip_index0 + i, step) only.  Enqueued on torch's current stream; no host sync.  boxes= (a `ctrlv_amd.boxes.BoxTable`
        on the device) with source_size=(Hs, Ws) instead of box_frames: the frames are rendered from the table first."""
        who = "TrainBatchPlan.prepare"
        dev = self.device
        if boxes is not None:
            # training from coordinates is a composition: ctrlv_box_frames_cond into the buffer box_frames points at, then the
            # call below on the same stream
            if box_frames is not None:
                raise ValueError(f"{who}: boxes and box_frames are mutually exclusive")
            if source_size is None:
                raise ValueError(f"{who}: boxes= needs source_size=(Hs, Ws), the size the coordinates refer to")
            from . import ops
            box_frames = ops.box_frames_cond(boxes, source_size, tuple(clips.shape[-2:]), dtype=self.dtype)
        for name, t in (("clips", clips), ("box_frames", box_frames)):
            if t is None:
                continue
            if t.dim() != 5 or t.shape[2] != 3 or t.dtype not in _DT:
                raise ValueError(f"{who}: {name} must be (n, F, 3, H, W) fp32 / fp16 / bf16")
            if not t.is_cuda or (t.device.index or 0) != (dev.index or 0):
                raise ValueError(f"{who}: {name} on {t.device}, the plans' weights on {dev}")
        if box_frames is not None and box_frames.shape != clips.shape:
            raise ValueError(f"{who}: box_frames {tuple(box_frames.shape)} must have the shape of clips {tuple(clips.shape)}")
        clips = clips.contiguous()
        box_frames = box_frames.contiguous() if box_frames is not None else None
        n, F, _, H, W = clips.shape
        L, D = self.vae._cfg.latent_channels, self.clip._cfg.projection_dim
        lat = (n, F, L, H // 8, W // 8)
        f32 = dict(dtype=torch.float32, device=dev)
        out = {"target_latents": torch.empty(lat, **f32), "noisy_latents": torch.empty(lat, **f32),
               "sample": torch.empty(n, F, 2 * L, H // 8, W // 8, dtype=sample_dtype or self.dtype, device=dev),
               "encoder_hidden_states": torch.empty(n, 1, D, dtype=self.dtype, device=dev),
               "sigmas": torch.empty(n, **f32), "timesteps": torch.empty(n, **f32),
               "indices": torch.empty(n, dtype=torch.int32, device=dev), "random_p": torch.empty(n, **f32)}
        if self._mode(mode) == 0:
            out["control_cond"] = torch.empty(lat, **f32)
        if return_noise:
            out["noise"] = torch.empty(lat, **f32)
        r = self.request(clips, box_frames, out, mode=mode, seed=seed, step=step, num_cond_frames=num_cond_frames,
                         dropout_prob=dropout_prob, scaling_factor=scaling_factor, clip_mean=clip_mean, clip_std=clip_std)
        need = self.workspace_bytes(r)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(self._lib.ctrlv_train_batch_prepare(self.vae._h, self.clip._h, ctypes.byref(r), self._ws.data_ptr(), self._ws.numel(),
                                                  stream), "ctrlv_train_batch_prepare")
        return out


_VAE_PLANS = {}


def vae_plan(vae, offset_limit_bytes=0, dtype=torch.bfloat16):
    """The `VaePlan` of an AutoencoderKLTemporalDecoder module, cached per object and keyed on the parameters' versions and
    storage (as the per-op executors' `_pack`): an in-place parameter update reloads the weights.  dtype: the plan's element
    type (bf16 for the module's own encode / decode routes)."""
    import weakref
    key = (id(vae), int(offset_limit_bytes)) if dtype == torch.bfloat16 else (id(vae), int(offset_limit_bytes), dtype)
    params = list(vae.parameters())
    ver = tuple(p._version for p in params) + (params[0].data_ptr(),)
    hit = _VAE_PLANS.get(key)
    if hit is not None and hit[0] == ver and hit[1]() is vae:
        return hit[2]
    plan = hit[2] if hit is not None and hit[1]() is vae and hit[2].device == params[0].device else \
        VaePlan(vae.config, params[0].device, offset_limit_bytes, dtype)
    plan.load_state_dict(vae.state_dict())
    _VAE_PLANS[key] = (ver, weakref.ref(vae), plan)
    return plan
