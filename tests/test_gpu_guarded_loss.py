"""Guard-band tests of the third binding table (include/unetpp_loss.h): loss_sums of unet_amd/loss.py between random guard
bytes, through the harness and the placements of tests/test_gpu_guarded.py, with its four assertions: guards intact, equal
to the NumPy form bit for bit, the same bits with the filling complemented, placements of one data set bitwise equal.  The
rows live in this module's own list (ROWS_LOSS); tests/test_loss_host.py compares it with the third table.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded_loss.py -m gpu"""
import numpy as np
import pytest

import guarded
import test_gpu_guarded as tg
from test_gpu_guarded import model, torch_cuda  # noqa: F401  (fixtures)
from unet_amd import loss as ls

# Symbols of the third table that write no caller-provided device buffer.
EXCLUDED_LOSS = {"unetpp_loss_layout": "layout query"}


def build_scene(C, logit_kind="plain", target_kind="plain"):
    def build(s, r):
        seed = int(r.integers(0, 1000))
        return {"logits": ls.make_logits(s[0], C, s[1], s[2], seed, logit_kind), "target": ls.make_target(s[0], C, s[1], s[2], seed, target_kind)}
    return build


def loss_row(name, C, gamma, **kinds):
    r = tg.Row(name, ["unetpp_loss_sums_f32"], build_scene(C, **kinds), lambda m, t, a: ls.loss_sums(m, t["logits"], t["target"], gamma),
               lambda a: ls.loss_sums_np(a["logits"], a["target"], gamma))
    r.classes = (C,)
    return r


ROWS_LOSS = [
    loss_row("loss_sums[3 classes]", 3, 2),
    loss_row("loss_sums[7 classes]", 7, 2),
    loss_row("loss_sums[3 classes, special pixels, gamma 3]", 3, 3, logit_kind="nonfinite", target_kind="out_of_range"),
]
ROW_BY_NAME = {r.name: r for r in ROWS_LOSS}


@pytest.mark.gpu
@pytest.mark.parametrize("placement", list(tg.PLACEMENTS))
@pytest.mark.parametrize("name", list(ROW_BY_NAME))
def test_row(torch_cuda, model, name, placement):  # noqa: F811
    r = ROW_BY_NAME[name]
    got = tg.run_row(torch_cuda, model, r, placement)
    if placement in tg.SAME_BITS:
        guarded.assert_same_bytes(tg.run_row(torch_cuda, model, r, tg.SAME_BITS[placement]), got,
                                  f"{name}: {tg.SAME_BITS[placement]} (aligned) against {placement} (the pointer says no)")
