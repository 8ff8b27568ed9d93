"""Best-of-N box candidates on the device (include/ctrlv_hip.h: ctrlv_best_candidate, ctrlv_gather_clips,
ctrlv_pipeline_best_boxes, ctrlv_pipeline_best_boxes_to_video; csrc/box_eval.hip, csrc/pipeline.hip): the two kernels against
their host restatements, the driver bit for bit against the same calls made by hand -- C predict_boxes, box_frames_post and
mask_counts calls, metrics.best_of on the host, one more box_frames_post --, the chain against best_boxes followed by generate,
one candidate against ctrlv_pipeline_boxes_to_video, and the seeded form against ctrlv_pipeline_prepare with call = c.  Models and
inputs are those of tests/test_pipeline_plan_gpu.py (tiny models, 3 frames x 128 x 192, 2 steps), reused by import."""
import ctypes

import pytest
import torch

from tests import box_eval_ref as E
from tests import guarded as Gd
from tests.test_pipeline_plan_gpu import DEV, F, H, STEPS, W, bits, build_setup, gen, same

pytestmark = pytest.mark.gpu
# The clean-up threshold of these tests: the channel sum of mid-grey, 3 x 127.5.  The tiny models have random weights and decode
# to frames around zero, i.e. around mid-grey: at the reference's 50 no pixel is dark, every candidate's mask is the whole frame
# and all scores tie; at mid-grey a good share of every frame's pixels is dark and the candidates' masks differ (checked below).
THRESHOLD = 382.5
K = 1
GUIDANCE = ((1.0, 2.0), (1.0, 3.0), (2.0, 4.0))
C = len(GUIDANCE)
KW = dict(noise_aug_strength=0.02, fps=7, motion_bucket_id=127, decode_chunk=2)
VIDEO_KW = dict(KW, min_guidance=1.0, max_guidance=3.0, conditioning_scale=0.8)
SEED = 0x5EEDB0C5


# ------------------------------------------------------------------------------------------------------------------ the kernels
def test_best_candidate_is_the_host_rule(hip_lib):
    """The crafted counts of tests/box_eval_ref.py, one case per clip of one call and each case alone: strictly best in the
    middle, a tie (the later wins), all unions zero, 1 / 3 against 2 / 6, and two 44-bit ratios that differ as rationals and
    round to one double."""
    from ctrlv_amd import metrics, ops
    names = [k for k in E.BEST_CASES if len(E.BEST_CASES[k][0]) == 3]
    batch = [[E.BEST_CASES[k][0][c][0] for k in names] for c in range(3)]                   # (3, n, 2, 3)
    want = [E.BEST_CASES[k][1][0] for k in names]
    assert metrics.best_of(batch) == want
    buf, flat = Gd.guarded_flat(len(names) * 4, torch.uint8, DEV)
    before = buf.clone()
    got = ops.best_candidate(torch.tensor(batch, dtype=torch.int64, device=DEV), out=flat.view(torch.int32))
    torch.cuda.synchronize()
    assert got.cpu().tolist() == want
    Gd.check_written_only_inside(before, buf, flat.view(1, -1), got.cpu().view(torch.uint8).view(1, -1), what="winner")
    for name, (counts, w) in E.BEST_CASES.items():
        t = torch.tensor(counts, dtype=torch.int64, device=DEV)
        assert ops.best_candidate(t).cpu().tolist() == w == metrics.best_of(t), name
    one = torch.tensor([[[[4, 4, 1], [0, 0, 0]]] * 300], dtype=torch.int64, device=DEV)     # C = 1, more clips than a workgroup
    assert ops.best_candidate(one).cpu().tolist() == [0] * 300


@pytest.mark.parametrize("per", [1, 15, 16, 4099])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
def test_gather_clips(hip_lib, per, aligned):
    """C = 3, n = 2: every pair of winners, an index outside [0, C) clamped into it, guard bands around the destination; the
    unaligned case puts source and destination at different offsets from a 16-byte boundary (3 and 5)."""
    from ctrlv_amd import ops
    n = 2
    src_buf = torch.empty(C * n * per + 64, dtype=torch.uint8, device=DEV)
    off = (-src_buf.data_ptr()) % 16 + (0 if aligned else 3)
    src = src_buf[off:off + C * n * per].view(C, n, per)
    src.copy_(torch.randint(0, 256, (C, n, per), generator=gen(per), dtype=torch.uint8))
    gap = 64 if aligned else 69
    for winners in ([0, 0], [1, 0], [2, 1], [0, 2], [-1, 7]):
        buf, flat = Gd.guarded_flat(n * per, torch.uint8, DEV, gap=gap)
        assert (flat.data_ptr() % 16 == 0) == aligned
        before = buf.clone()
        got = ops.gather_clips(src, torch.tensor(winners, dtype=torch.int32, device=DEV), out=flat.view(n, per))
        torch.cuda.synchronize()
        want = torch.stack([src[min(max(w, 0), C - 1), i] for i, w in enumerate(winners)])
        assert torch.equal(got, want), (per, aligned, winners)
        Gd.check_written_only_inside(before, buf, flat.view(1, -1), want.view(1, -1), what=f"gather {per} {winners}")
    if per == 4099 and not aligned:            # equal offsets: 16-byte units between a head and a tail of single bytes
        buf, flat = Gd.guarded_flat(n * per, torch.uint8, DEV, gap=67)
        assert flat.data_ptr() % 16 == src.data_ptr() % 16 == 3
        before = buf.clone()
        got = ops.gather_clips(src, torch.tensor([2, 0], dtype=torch.int32, device=DEV), out=flat.view(n, per))
        want = torch.stack([src[2, 0], src[0, 1]])
        assert torch.equal(got, want)
        Gd.check_written_only_inside(before, buf, flat.view(1, -1), want.view(1, -1), what="gather head / tail")
    wide = torch.randn(C, n, 3, 5, generator=gen(1)).to(DEV)                                 # any dtype, any trailing shape
    assert torch.equal(ops.gather_clips(wide, torch.tensor([1, 2], dtype=torch.int32, device=DEV)), torch.stack([wide[1, 0], wide[2, 1]]))


# ------------------------------------------------------------------------------------------------------------------- the driver
@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def el(request, hip_lib):
    return request.param


@pytest.fixture(scope="module")
def setup(el):
    s = build_setup(el)
    g0 = gen(23)
    s.cand_lat = [(torch.randn(2, F, 4, H // 8, W // 8, generator=g0) * s.sched.init_noise_sigma).to(DEV) for _ in GUIDANCE]
    s.cand_aug = [torch.randn(2, 3, H, W, generator=g0).to(DEV) for _ in GUIDANCE]
    s.hand = {}
    return s


def _inputs(s, n):
    return [t[:n].contiguous() for t in s.cand_lat], [t[:n].contiguous() for t in s.cand_aug]


def _hand(s, n):
    """Stage 1 by hand, once per n: candidate c's decoded frames (n F, 3, H, W) and cleaned frames (n, F, 3, H, W)."""
    from ctrlv_amd import ops
    if n not in s.hand:
        lats, augs = _inputs(s, n)
        frames, clean = [], []
        for c, (lo, hi) in enumerate(GUIDANCE):
            _, fr, _ = s.pipe_svd.predict_boxes(s.image[:n], lats[c], s.sigmas, s.timesteps, s.cond[:n], K, aug_noise=augs[c],
                                                frames_u8=False, min_guidance=lo, max_guidance=hi, **KW)
            frames.append(fr.clone())
            clean.append(ops.box_frames_post(fr, F, THRESHOLD, pt=False, cond=False)[2])
        torch.cuda.synchronize()
        s.hand[n] = (frames, clean)
    return s.hand[n]


def _expect(s, n, gt):
    """The rest by hand: the counts, the host's choice, the winner's frames gathered on the host, post-processed."""
    from ctrlv_amd import metrics, ops
    frames, clean = _hand(s, n)
    counts = torch.stack([ops.mask_counts(gt, clean[c]) for c in range(C)])
    winners = metrics.best_of(counts)
    gathered = torch.cat([frames[w][i * F:(i + 1) * F] for i, w in enumerate(winners)])
    pt, cond, u8 = ops.box_frames_post(gathered, F, THRESHOLD)
    torch.cuda.synchronize()
    return pt, cond, u8, winners, counts


def _best(s, n, gt, **kw):
    lats, augs = _inputs(s, n)
    out = s.pipe_svd.best_boxes(s.image[:n], s.cond[:n], gt, GUIDANCE, K, latents=lats, aug_noise=augs,
                                schedule=(s.sigmas, s.timesteps), clean_threshold=THRESHOLD, **dict(KW, **kw))
    torch.cuda.synchronize()
    return out


def _same_five(got, want, n):
    for a, b, what in zip(got[:3], want[:3], ("out_pt", "out_cond", "out_u8")):
        assert a.shape == b.shape and a.dtype == b.dtype, what
        assert torch.equal(bits(a), bits(b)), what
    assert got[3].dtype == torch.int32 and got[3].cpu().tolist() == want[3]
    assert got[4].shape == (C, n, 2, 3) and torch.equal(got[4], want[4])


def _ground_truths(s, n):
    _, clean = _hand(s, n)
    masks = [(clean[c] != 0).any(dim=2) for c in range(C)]                              # (n, F, H, W)
    for c in range(C):
        share = [float(masks[c][i].float().mean()) for i in range(n)]
        print(f"  n={n} candidate {c}: share of pixels in the mask per clip {[round(v, 3) for v in share]}")
        assert all(0.02 < v < 0.98 for v in share), "a candidate's mask is (nearly) empty or full: the scores would all tie"
        for d in range(c):
            assert all(not torch.equal(masks[c][i], masks[d][i]) for i in range(n)), "two candidates predict the same mask"
    crossed = torch.stack([clean[1][0], clean[0][1]]) if n == 2 else clean[1][:1].clone()
    return {"crossed": (crossed, [1, 0][:n]), "zeros": (torch.zeros_like(clean[0]), [C - 1] * n),
            "candidate0": (clean[0].clone(), [0] * n)}


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("which", ["crossed", "zeros", "candidate0"])
def test_best_boxes_is_the_calls_made_by_hand(setup, n, which):
    """Three ground truths.  crossed: clip 0 is candidate 1's cleaned frames and clip 1 candidate 0's -- the winners are (1, 0):
    the middle candidate, and a different one per clip.  zeros: every IoU is 0 and the tie goes to the last candidate (the
    predictions are checked to be non-empty first).  candidate0: only candidate 0 scores 1."""
    gt, winners = _ground_truths(setup, n)[which]
    want = _expect(setup, n, gt)
    assert want[3] == winners, (which, want[3], want[4].cpu().tolist())
    got = _best(setup, n, gt)
    _same_five(got, want, n)
    assert bool(got[2].any()) and float(got[0].float().min()) >= 0.0 and float(got[0].float().max()) <= 1.0


def test_best_boxes_without_frame_outputs_and_the_scores(setup):
    """pt / cond / u8 not asked for: the gather and the last post are skipped, winner and counts are the same; the counts give
    the triples eval_overall.py logs."""
    from ctrlv_amd import metrics
    gt, winners = _ground_truths(setup, 2)["crossed"]
    want = _expect(setup, 2, gt)
    got = _best(setup, 2, gt, pt=False, cond=False, u8=False)
    assert got[:3] == (None, None, None) and got[3].cpu().tolist() == winners and torch.equal(got[4], want[4])
    scores = metrics.candidate_scores(got[4])
    assert scores[1][0][0][0] == 1.0 and scores[0][1][0][0] == 1.0                       # the crossed candidates match exactly
    assert all(0.0 <= scores[c][i][k][0] <= 1.0 for c in range(C) for i in range(2) for k in range(2))


def _chain(s, n, gt, guidance=GUIDANCE, **kw):
    from ctrlv_amd.plan import best_boxes_to_video
    lats, augs = _inputs(s, n)
    sched = (s.sigmas, s.timesteps)
    args = dict(box_latents=lats[:len(guidance)], video_latents=s.lat[:n], box_schedule=sched, video_schedule=sched,
                box_aug_noise=augs[:len(guidance)], video_aug_noise=s.aug[:n], clean_threshold=THRESHOLD, box_kw=KW, video_kw=VIDEO_KW)
    out = best_boxes_to_video(s.pipe_svd, s.pipe, s.image[:n], s.cond[:n], gt, guidance, K, **dict(args, **kw))
    torch.cuda.synchronize()
    return out


def test_the_chain_is_best_boxes_then_generate(setup):
    s, n = setup, 2
    gt, winners = _ground_truths(s, n)["crossed"]
    pt, cond, u8, w, counts = _best(s, n, gt)
    want = s.pipe.generate(s.image[:n], s.lat[:n], s.sigmas, s.timesteps, cond=cond.view(n, F, 3, H, W), aug_noise=s.aug[:n],
                           **VIDEO_KW)
    torch.cuda.synchronize()
    got = _chain(s, n, gt)
    same(got[:3], want)
    assert torch.equal(got[3], u8) and got[4].cpu().tolist() == winners == w.cpu().tolist() and torch.equal(got[5], counts)


def test_one_candidate_is_boxes_to_video(setup):
    """C = 1: the bits of ctrlv_pipeline_boxes_to_video (the copy through the gather changes nothing)."""
    from ctrlv_amd.plan import boxes_to_video
    s, n = setup, 1
    lats, augs = _inputs(s, n)
    sched = (s.sigmas, s.timesteps)
    want = boxes_to_video(s.pipe_svd, s.pipe, s.image[:n], lats[1], s.lat[:n], sched, sched, s.cond[:n], K, box_aug_noise=augs[1],
                          video_aug_noise=s.aug[:n], clean_threshold=THRESHOLD,
                          box_kw=dict(KW, min_guidance=GUIDANCE[1][0], max_guidance=GUIDANCE[1][1]), video_kw=VIDEO_KW)
    torch.cuda.synchronize()
    gt = torch.zeros(n, F, 3, H, W, dtype=torch.uint8, device=DEV)
    got = _chain(s, n, gt, guidance=GUIDANCE[1:2], box_latents=lats[1:2], box_aug_noise=augs[1:2])
    same(got[:3], want[:3])
    assert torch.equal(got[3], want[3]) and got[4].cpu().tolist() == [0] and got[5].shape == (1, n, 2, 3)


def test_the_seeded_form_is_prepare_with_call_c(setup):
    """seed=: candidate c's latents and aug_noise are the draws of call = c, stage 2's those of call = C, the schedule the
    library's -- fed by hand through ops.randn and euler_schedule the unseeded calls give the same bits."""
    from ctrlv_amd import ops
    from ctrlv_amd.plan import best_boxes_to_video, euler_schedule
    s, n = setup, 2
    sig, ts, ins = euler_schedule(STEPS)
    draw = lambda call: (ops.randn(SEED, (n, 3, H, W), clip0=3, call=call, stream_id=0, device=DEV),           # noqa: E731
                         ops.randn(SEED, (n, F, 4, H // 8, W // 8), clip0=3, call=call, stream_id=1, scale=ins, round_el=True,
                                   el=s.el, device=DEV))
    augs, lats = zip(*(draw(c) for c in range(C + 1)))
    gt = _ground_truths(s, n)["crossed"][0]
    image, boxes = s.image[:n], s.cond[:n]
    want = s.pipe_svd.best_boxes(image, boxes, gt, GUIDANCE, K, latents=lats[:C], aug_noise=augs[:C], schedule=(sig, ts),
                                 clean_threshold=THRESHOLD, **KW)
    got = s.pipe_svd.best_boxes(image, boxes, gt, GUIDANCE, K, seed=SEED, num_steps=STEPS, clip_index0=3,
                                clean_threshold=THRESHOLD, **KW)
    torch.cuda.synchronize()
    _same_five(got, (want[0], want[1], want[2], want[3].cpu().tolist(), want[4]), n)
    assert bool(torch.isfinite(got[0].float()).all())
    sched = (sig, ts)
    want = best_boxes_to_video(s.pipe_svd, s.pipe, image, boxes, gt, GUIDANCE, K, box_latents=lats[:C], video_latents=lats[C],
                               box_schedule=sched, video_schedule=sched, box_aug_noise=augs[:C], video_aug_noise=augs[C],
                               clean_threshold=THRESHOLD, box_kw=KW, video_kw=VIDEO_KW)
    got = best_boxes_to_video(s.pipe_svd, s.pipe, image, boxes, gt, GUIDANCE, K, seed=SEED, num_steps=STEPS, clip_index0=3,
                              clean_threshold=THRESHOLD, box_kw=KW, video_kw=VIDEO_KW)
    torch.cuda.synchronize()
    same(got[:3], want[:3])
    assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4]) and torch.equal(got[5], want[5])


def test_workspace_queries_and_the_too_small_workspace(setup):
    """Both queries answer the size their call accepts: one byte less is CTRLV_E_WORKSPACE with the needed size in the message
    and nothing launched; with exactly that size, 4 KiB of pattern behind the workspace survive and the bits are the same."""
    from ctrlv_amd import _lib
    s, n = setup, 1
    lib = s.pipe._lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gt = _ground_truths(s, n)["crossed"][0]
    want = _expect(s, n, gt)
    lats, augs = _inputs(s, n)
    q, keep, out = s.pipe_svd.best_boxes_request("test", s.image[:n], s.cond[:n], gt, GUIDANCE, K, latents=lats, aug_noise=augs,
                                                 schedule=(s.sigmas, s.timesteps), clean_threshold=THRESHOLD, **KW)
    for t in out:
        t.zero_()
    need = lib.ctrlv_pipeline_best_boxes_workspace_bytes(s.pipe_svd._h, ctypes.byref(q))
    assert need > 0 and need % 256 == 0, _lib.last_error(lib)
    buf = torch.empty(need + 4096, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf[need:] = 0xA5
    torch.cuda.synchronize()
    assert lib.ctrlv_pipeline_best_boxes(s.pipe_svd._h, ctypes.byref(q), buf.data_ptr(), need - 1, st) == -5
    assert str(need) in _lib.last_error(lib) and "ws_bytes" in _lib.last_error(lib)
    torch.cuda.synchronize()
    assert not bool(out[2].any()) and not bool(out[4].any())
    assert lib.ctrlv_pipeline_best_boxes(s.pipe_svd._h, ctypes.byref(q), buf.data_ptr(), need, st) == 0, _lib.last_error(lib)
    torch.cuda.synchronize()
    _same_five(out, want, n)
    assert bool((buf[need:] == 0xA5).all())

    from ctrlv_amd.plan import PipelinePlan                                      # the chain's query and call
    qc = _lib.BestChainRequest()
    out_lat = torch.full_like(s.lat[:n], 7.0)
    rv, kv = s.pipe.request(s.image[:n].contiguous(), s.lat[:n].contiguous(), s.sigmas, s.timesteps, aug_noise=s.aug[:n].contiguous(),
                            out_latents=out_lat, **VIDEO_KW)
    qc.boxes, qc.video = q, rv
    assert isinstance(s.pipe, PipelinePlan)
    need_c = lib.ctrlv_pipeline_best_chain_workspace_bytes(s.pipe_svd._h, s.pipe._h, ctypes.byref(qc))
    assert need_c >= need and need_c % 256 == 0, _lib.last_error(lib)
    ws = torch.empty(need_c, dtype=torch.uint8, device=DEV)
    assert lib.ctrlv_pipeline_best_boxes_to_video(s.pipe_svd._h, s.pipe._h, ctypes.byref(qc), ws.data_ptr(), need_c - 1, st) == -5
    assert str(need_c) in _lib.last_error(lib) and "ws_bytes" in _lib.last_error(lib)
    torch.cuda.synchronize()
    assert bool((out_lat == 7.0).all())
    qc.video.num_frames = F - 1
    assert lib.ctrlv_pipeline_best_chain_workspace_bytes(s.pipe_svd._h, s.pipe._h, ctypes.byref(qc)) == 0
    assert "geometry" in _lib.last_error(lib)
    del keep, kv
