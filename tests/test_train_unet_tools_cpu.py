"""CPU checks of the stage-1 tools: the analytic work of tools/train_unet_bench.py is counted from the layer list (the
oracle UNet on the meta device), and tools/wgrad_bench.py carries the three upsampler rows next to its cfg5 rows."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_train_unet_bench_analytic_work():
    import train_unet_bench as tb
    f_all, b_all = tb.analytic_tflop(25, 72, 128, "all")
    f_tmp, b_tmp = tb.analytic_tflop(25, 72, 128, "temporal")
    # the UNet forward at 576 x 1024, 25 frames is SURVEY's 80 TFLOP; all-mode backward = dgrad + wgrad of every layer
    assert 78.0 < f_all < 82.0 and f_tmp == f_all
    assert 1.9 * f_all < b_all < 2.1 * f_all
    assert f_all < b_tmp < b_all                     # temporal-only: dgrad everywhere, wgrad of the temporal blocks only
    f_s, b_s = tb.analytic_tflop(25, 40, 64, "all")
    assert 0.2 * f_all < f_s < 0.35 * f_all and b_s < b_all


def test_wgrad_bench_upsampler_rows():
    import wgrad_bench as wb
    rows = wb.shapes()
    up = [r for r in rows if " x2 " in r[0]]
    assert [(r[2], r[5]) for r in up] == [(1280, (9, 16, 18, 32)), (1280, (18, 32, 36, 64)), (640, (36, 64, 72, 128))]
    assert all(r[1] == 25 * r[5][2] * r[5][3] and r[4] == 9 for r in up)
    assert len(rows) == 21 + 3 and rows[-3:] == up
