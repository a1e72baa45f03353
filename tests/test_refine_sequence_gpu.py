"""The ORDER of the library calls that ``RefineBatch.run()`` issues, pinned per configuration: room 0 of tests/golden/refine_loop.npz at
96 x 96, two iterations.  The lists were recorded from the loop as it stood before its set-up was restructured (one room start, one target
build, one capture helper, ``_forward_to_placement``); a change of the loops that moves, adds or drops a call shows here first.
Part of what is pinned: the first run's prefix (``_first_iterate_sizes``: decoder, optional head, placement) and, under capture, iteration 0
issued twice (the warm-up on a side stream, then the recording) while iteration 1 - a replay - issues nothing."""
import pytest

from conftest import load_golden, pkg

import test_refine_report_gpu as RR

pytestmark = pytest.mark.gpu

ITERS = 2

PREFIX = ["sln_vae_group_decoder", "sln_place_forward_rooms"]
FORWARD = ["sln_vae_group_decoder", "sln_place_forward_rooms", "sln_scene_forward_live", "sln_refine_loss_forward"]
BACKWARD = ["sln_refine_loss_backward", "sln_scene_backward", "sln_place_backward_rooms", "sln_vae_group_decoder_backward", "sln_refine_sgd_rooms"]
REPORTED = (["sln_vae_group_decoder", "sln_place_forward_rooms", "sln_layout_cuboid_iou", "sln_scene_forward_live", "sln_refine_loss_forward",
             "sln_refine_report"] + BACKWARD)
PICTURED = FORWARD + ["sln_scene_pictures"] + BACKWARD
HEAD_PREFIX = ["sln_vae_group_decoder", "sln_refine_head_forward_rooms", "sln_place_forward_rooms"]
HEAD_ITERATION = (["sln_vae_group_decoder", "sln_refine_head_forward_rooms", "sln_place_forward_rooms", "sln_scene_forward_live",
                   "sln_refine_loss_forward", "sln_refine_loss_backward", "sln_scene_backward", "sln_place_backward_rooms",
                   "sln_refine_head_backward_rooms", "sln_vae_group_decoder_backward", "sln_refine_sgd_rooms"])

EXPECTED = {
    "default": PREFIX + (FORWARD + BACKWARD) * 2,
    "report": PREFIX + REPORTED * 2,
    "pictures": PREFIX + PICTURED * 2,
    "separate_head": HEAD_PREFIX + HEAD_ITERATION * 2,
    "capture": PREFIX + (FORWARD + BACKWARD) * 2,          # warm-up + recording of iteration 0; iteration 1 replays
}
CONFIGS = {"default": {}, "report": dict(report="all"), "pictures": dict(pictures="all"), "separate_head": {}, "capture": {}}


class _Ordered:
    """the loaded library behind a proxy that lists every entry point looked up, in order (the ordered variant of
    test_refine_report_gpu's counting proxy: the loop looks an entry point up once per call, inside run())"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self.real, name)


@pytest.mark.parametrize("config", list(EXPECTED))
def test_refine_batch_call_sequence(config, monkeypatch):
    R, Lm = pkg("host.refine"), pkg("_lib")
    if config == "separate_head":
        monkeypatch.setenv("SLN_REFINE_SEPARATE_HEAD", "1")
    g = load_golden("refine_loop")
    model = RR._loop_model(g, "refine_loop")
    rb = R.RefineBatch(model, RR._loop_rooms(g, [0]), bank=RR._bank(g), image_size=RR.LOOP_IMAGE, iters=ITERS, **CONFIGS[config])
    try:
        real = Lm.lib()
        Lm._lib = proxy = _Ordered(real)
        try:
            rb.run(capture=config == "capture")
        finally:
            Lm._lib = real
    finally:
        rb.close()
    print("%s: %s" % (config, proxy.calls))
    assert proxy.calls == EXPECTED[config]
