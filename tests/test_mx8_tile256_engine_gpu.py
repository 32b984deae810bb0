"""EngineOptions.mx8_tile256 on a real MI355X: with mx8_forward on, the MX GEMMs that lpi_gemm_mx8_256_ok takes go out on the phased 256x256 tile and
everything the engine computes stays the same bits; training and the option-off engine never see the switch.

Configuration: three-layer towers of width 256 (4 heads of 64), so N and K of the block GEMMs are 256, 768 and 1024 — all multiples of 256.  The engine
pads a tower's rows to whole 256-row tiles (Tower.workspace): 4 images of 32 x 32 at patch 16 are 4 x (1 class + 4 patch + the prompt) rows, a few dozen,
padded to 256; the text tower's ragged rows (at most 4 x 77) pad to 256 or 512 — the test asserts the multiple of 256 on every request.  Two full blocks
per tower take the MX path, the pooled last block stays on the 2-byte kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lpi_amd import _lib, synth  # noqa: E402
from lpi_amd import engine as E  # noqa: E402
from lpi_amd.engine import DualEncoder, EngineOptions, PackedIds  # noqa: E402
from lpi_amd.functional import DecomposedPromptFn  # noqa: E402
from lpi_amd.step import _CP_ORDER, train_step  # noqa: E402
from lpi_amd.synth import ClipConfig  # noqa: E402

DEV = "cuda:0"
W256 = ClipConfig("tiny3w256", 256, 32, 3, 256, 16, 77, 49408, 256, 4, 3)
MX_NAMES = ("lpi_gemm_nt_mx8", "lpi_gemm_nt_mx8_256")


def encodes(cfg, sd, fac, img, ids, **opts):
    """Features of the train=False encodes with prompts, the launches they took, and per MX GEMM request (padded shape, kind the library reports)."""
    enc = DualEncoder(cfg, sd, dtype="bf16", device=DEV, options=EngineOptions(**opts))
    with torch.no_grad():
        vis, txt = DecomposedPromptFn.apply(*[fac[k] for k in _CP_ORDER], 1.0, None)
    lib, log, issue = _lib.load(), [], E.Mx8Req.issue

    def logged(self):
        issue(self)
        if self.name in MX_NAMES:
            log.append((self.name, tuple(self.args[1:4]), int(lib.lpi_gemm_last_kernel())))
    E.Mx8Req.issue = logged
    try:
        n0 = _lib.launch_count()
        fi = enc.encode_image(img, vis, 2, train=False)
        ft = enc.encode_text(PackedIds(ids).to(DEV), txt, 2, train=False)
        torch.cuda.synchronize()
        launches = _lib.launch_count() - n0
    finally:
        E.Mx8Req.issue = issue
    return fi.cpu(), ft.cpu(), launches, log


@pytest.fixture(scope="module")
def setup():
    cfg = W256
    sd = synth.clip_state_dict(cfg)
    fac = {k: torch.from_numpy(v).to(DEV) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
    img = torch.from_numpy(synth.images(4, cfg.image_resolution)).to(DEV)
    return cfg, sd, fac, img, synth.token_ids(4)


def test_same_bits_and_launches_as_the_128x128_arm(setup):
    lib = _lib.load()
    on = encodes(*setup, mx8_forward=True)
    off = encodes(*setup, mx8_forward=True, mx8_tile256=False)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert on[2] == off[2]
    # the other arm issues the parent's calls
    assert len(off[3]) == 2 * 2 * 4 and all(name == "lpi_gemm_nt_mx8" and kind == _lib.GEMM_K_MX8 for name, _, kind in off[3])
    # this arm: the 256x256 kernel wherever the predicate takes the padded shape, the 128x128 kernel everywhere else
    assert [shape for _, shape, _ in on[3]] == [shape for _, shape, _ in off[3]]
    want = [_lib.GEMM_K_MX8_256 if lib.lpi_gemm_mx8_256_ok(*shape) else _lib.GEMM_K_MX8 for _, shape, _ in on[3]]
    assert [kind for _, _, kind in on[3]] == want
    # the vision tower's eight block GEMMs (256 padded rows; N, K in {256, 768, 1024}) all pass
    assert all(M % 256 == 0 for _, (M, _, _), _ in on[3])
    assert want[:8] == [_lib.GEMM_K_MX8_256] * 8
    assert np.isfinite(on[0].float().numpy()).all() and np.isfinite(on[1].float().numpy()).all()


def test_towers_the_predicate_refuses_stay_on_the_128x128_kernel(setup):
    """Width 128 (tests/test_mx8_engine_gpu.py's towers): no N or K is a multiple of 256, so the default mx8_tile256=True changes no call."""
    cfg = ClipConfig("tiny3", 128, 32, 3, 128, 16, 77, 49408, 128, 2, 3)
    _, _, _, img, ids = setup
    sd = synth.clip_state_dict(cfg)
    fac = {k: torch.from_numpy(v).to(DEV) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
    log = encodes(cfg, sd, fac, img, ids, mx8_forward=True)[3]
    assert len(log) == 16 and all(name == "lpi_gemm_nt_mx8" and kind == _lib.GEMM_K_MX8 for name, _, kind in log)


def _train(cfg, sd, img, ids, **opts):
    enc = DualEncoder(cfg, sd, dtype="bf16", device=DEV, options=EngineOptions(**opts))
    fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
    if opts.get("mx8_forward"):      # a no-grad forward first: its MX launches must leave the training arena alone
        enc.encode_image(img, None, 1, train=False)
    n0 = _lib.launch_count()
    out = train_step(enc, img, PackedIds(ids, 17).to(DEV), fac, 2)
    torch.cuda.synchronize()
    launches = _lib.launch_count() - n0
    return ({**{k: out[k].detach().cpu() for k in ("img_f", "txt_f", "base_loss", "alignment_loss")},
             **{"grad." + k: fac[k].grad.cpu() for k in synth.PROMPT_NAMES}}, launches)


def test_train_step_never_takes_the_path(setup):
    cfg, sd, _, img, ids = setup
    ref, n_ref = _train(cfg, sd, img, ids)
    got, n_got = _train(cfg, sd, img, ids, mx8_forward=True, mx8_tile256=True)
    assert n_got == n_ref and set(got) == set(ref) and len(ref) == 9
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


def test_without_mx8_forward_the_switch_changes_nothing(setup):
    a = encodes(*setup, mx8_tile256=True)
    b = encodes(*setup, mx8_tile256=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3] == []
