"""CPU reference of the FP8 feed-forward mode (include/ctrlv_hip.h, "FP8 linear GEMM").

`quant_rows(x)` is the numerical contract of ctrlv_quant_rows_f8 written with torch.float8_e4m3fn: one scale per row,
s = max|x| / 448 (1 for an all-zero row, never below the smallest normal fp32), codes = e4m3(x / s), round-to-nearest-even,
saturating.  `fake_quant_feed_forwards(module, served)` puts that quantisation in front of both linears of every oracle
`FeedForward` the mode serves (activation rows by a forward pre-hook, weight rows in place), so that the oracle computes, in
fp32 arithmetic, what the HIP path computes on e4m3 operands.  Nothing under oracle/ is changed: the hooks live on the module
instances the caller passes (pass a copy).
"""
import torch

F8_MAX = 448.0
_TINY = torch.finfo(torch.float32).tiny


def quant_rows(x):
    """x [..., K] -> (codes: torch.float8_e4m3fn of x's shape, scale: fp32 x.shape[:-1])."""
    x = x.detach().float()
    a = x.abs().amax(dim=-1, keepdim=True)
    s = torch.where(a > 0, (a / F8_MAX).clamp_min(_TINY), torch.ones_like(a))
    q = (x / s).clamp(-F8_MAX, F8_MAX).to(torch.float8_e4m3fn)
    return q, s.squeeze(-1)


def fake_quant(x):
    """x with every row replaced by its dequantised e4m3 codes (fp32)."""
    q, s = quant_rows(x)
    return q.float() * s.unsqueeze(-1)


def served_dim(dim):
    """The feed-forwards ctrlv_gemm_f8_serves accepts: both contractions (dim and 4 dim) multiples of 128."""
    return dim % 128 == 0 and 4 * dim <= 5120


def fake_quant_feed_forwards(module, served=served_dim):
    """Fake-quantise, in place, both linears of every `FeedForward` under `module` whose input width `served` accepts.
    Returns the number of feed-forwards wrapped."""
    import ctrlv_ref.blocks as RB
    n = 0
    for ff in module.modules():
        if not isinstance(ff, RB.FeedForward):
            continue
        proj, out = ff.net[0].proj, ff.net[2]
        if not served(proj.in_features):
            continue
        for lin in (proj, out):
            with torch.no_grad():
                lin.weight.copy_(fake_quant(lin.weight))
            lin.register_forward_pre_hook(lambda m, args: (fake_quant(args[0]),) + tuple(args[1:]))
        n += 1
    return n


def oracle_pair(config, seed=0, dtype=torch.bfloat16, zero_conv_std=0.02):
    """The oracle half of tests/parity_utils.make_pair: (unet, controlnet) with the seeded parameters rounded to `dtype`."""
    import ctrlv_ref as R
    ou = R.UNetSpatioTemporalConditionModel(**config)
    R.seeded_init_(ou, seed)
    oc = R.ControlNetModel.from_unet(ou)
    R.seeded_init_(oc, seed + 1, zero_conv_std=zero_conv_std)
    for m in (ou, oc):
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(p.to(dtype).float())
        m.eval()
    return ou, oc


def quantised_copy(ou, oc, served=served_dim):
    """Deep copies of an oracle pair with the served feed-forwards fake-quantised; (unet, controlnet, n_wrapped)."""
    import copy
    qu, qc = copy.deepcopy(ou), copy.deepcopy(oc)
    n = fake_quant_feed_forwards(qu, served) + fake_quant_feed_forwards(qc, served)
    return qu, qc, n


def errors(got, ref):
    """rel-L2 of (unet output, mid residual, worst down residual) between two parity_utils forward dicts."""
    from tests.parity_utils import rel_l2
    return dict(unet=rel_l2(got["unet"], ref["unet"]), mid=rel_l2(got["mid"], ref["mid"]),
                down=max(rel_l2(a, b) for a, b in zip(got["down"], ref["down"])))
