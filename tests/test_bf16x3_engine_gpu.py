"""EngineOptions.gemm_bf16x3 on a real MI355X: with the option off the f32 engine is the default engine bit for bit; with it on the towers' GEMMs that go to
lpi_gemm_nt run the split-bf16 kernels (and say so through lpi_gemm_last_kernel) while the few-row GEMMs stay on the exact f32 kernel, launch count
unchanged; accuracy against the option-off f32 engine next to the bf16 engine's; the plugin and the engine against the reference's fixtures.

Which GEMMs take the new path is a rule of SHAPE (engine._few_rows: at most 512 padded rows -> lpi_gemm_nt_rows, exact f32).  With the tiny three-layer
towers at 4 pairs every GEMM of a step has at most 512 rows (vision 4 x 21 -> 256, text 4 x 77 -> 512): the option then changes nothing, which the
4-pair case asserts; at 8 pairs the text tower (8 x 77 -> 768 rows) takes the bf16x3 kernels while the vision tower stays few-row, and that case carries
the accuracy and attribution assertions on a path that really ran.  The same holds for fixture tiny_d1 (4 pairs): its figures are the f32 kernels'; the
reference comparison that exercises the new kernels is the ViT-B/16 fixture vitb16_d1."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lpi_amd import _lib, synth  # noqa: E402
from lpi_amd import engine as E  # noqa: E402
from lpi_amd.engine import DualEncoder, EngineOptions  # noqa: E402
from lpi_amd.functional import DecomposedPromptFn  # noqa: E402
from lpi_amd.step import _CP_ORDER, train_step  # noqa: E402
from lpi_amd.synth import ClipConfig  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY3 = ClipConfig("tiny3", 128, 32, 3, 128, 16, 77, 49408, 128, 2, 3)      # the towers of tests/test_mx8_engine_gpu.py
DEPTH = 2
GRADS = ["grad." + k for k in synth.PROMPT_NAMES]
MIN_GRAD_COSINE = 0.99999

# Against the reference's fixtures with the option on, measured on the first MI355X run ("bf16x3 GEMMs"); the bars are 2 x these.
# The f32 mode's own bars are 1e-4 on the logits and 1e-3 max|ref| + 1e-5 on the factor gradients (tests/test_plugin_gpu.py, tests/test_model_gpu.py).
MEASURED = {
    "tiny_d1": {"logits": 1.982e-06, "grads": 2.258e-06},      # every GEMM of this fixture is few-row: the f32 kernels' figures (module docstring)
    "vitb16_d1": {"logits": 1.311e-05, "grads": 8.418e-05},    # meets the f32 bars with a factor 7.6 / 11.9 to spare
}


def run(cfg, sd, dtype, pairs, options=None, profile=False):
    """One train_step and one train=False encode of the same inputs.  -> dict of host arrays, launches of the step, GEMM kernel kinds of the step."""
    enc = DualEncoder(cfg, sd, dtype=dtype, device=DEV, options=options)
    fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
    img = torch.from_numpy(synth.images(pairs, cfg.image_resolution)).to(DEV)
    ids = torch.from_numpy(synth.token_ids(pairs)).to(DEV)
    n0 = _lib.launch_count()
    out = train_step(enc, img, ids, fac, DEPTH)
    torch.cuda.synchronize()
    launches = _lib.launch_count() - n0
    res = {k: out[k].detach().float().cpu().numpy() for k in ("img_f", "txt_f", "base_loss", "alignment_loss")}
    res["logits"] = (enc.logit_scale_exp * out["img_f"].float() @ out["txt_f"].float().t()).cpu().numpy()
    for k in synth.PROMPT_NAMES:
        res["grad." + k] = fac[k].grad.float().cpu().numpy()
    with torch.no_grad():
        vis, txt = DecomposedPromptFn.apply(*[fac[k].detach() for k in _CP_ORDER], 1.0, None)
        res["enc_img"] = enc.encode_image(img, vis, DEPTH, train=False).float().cpu().numpy()
        res["enc_txt"] = enc.encode_text(ids, txt, DEPTH, train=False).float().cpu().numpy()
    torch.cuda.synchronize()
    kinds = []
    if profile:      # a second step for the kernel kinds alone: the bracketing events change how the loss issues its own GEMMs, so it is not the counted one
        E.GEMM_PROFILE = []
        try:
            train_step(enc, img, ids, fac, DEPTH)
            torch.cuda.synchronize()
            kinds = [p[4] for p in E.GEMM_PROFILE]
        finally:
            E.GEMM_PROFILE = None
    return res, launches, kinds


_RUNS = {}


def runs(pairs):
    """The four engines on the same inputs, once per batch size: default f32, f32 with the option off, f32 with it on, bf16."""
    if pairs not in _RUNS:
        sd = synth.clip_state_dict(TINY3)
        _RUNS[pairs] = {
            "default": run(TINY3, sd, "f32", pairs, None),
            "off": run(TINY3, sd, "f32", pairs, EngineOptions(gemm_bf16x3=False), profile=True),
            "on": run(TINY3, sd, "f32", pairs, EngineOptions(gemm_bf16x3=True), profile=True),
            "bf16": run(TINY3, sd, "bf16", pairs, None),
        }
    return _RUNS[pairs]


def maxerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("pairs", [4, 8])
def test_option_off_is_the_default_engine(pairs):
    r = runs(pairs)
    (d, nd, _), (o, no, _) = r["default"], r["off"]
    assert set(d) == set(o)
    for k in d:
        assert np.array_equal(d[k], o[k]), k
    assert nd == no
    assert _lib.GEMM_K_X3 not in r["off"][2]


@pytest.mark.parametrize("pairs", [4, 8])
def test_option_on_launches_and_kernels(pairs):
    r = runs(pairs)
    (off, n_off, k_off), (on, n_on, k_on) = r["off"], r["on"]
    assert n_on == n_off and len(k_on) == len(k_off)
    assert _lib.GEMM_K_ROWS in k_on      # the few-row GEMMs stay where they were
    few = _lib.GEMM_K_ROWS
    assert [k == few for k in k_on] == [k == few for k in k_off]
    # a bf16x3 launch of the on engine is an lpi_gemm_nt launch of a tower in the off engine; everything else is the same kernel in both
    for a, b in zip(k_on, k_off):
        assert (b in (_lib.GEMM_K_128, _lib.GEMM_K_256)) if a == _lib.GEMM_K_X3 else a == b
    # the shape rule: no GEMM of the 4-pair step has more than 512 padded rows (module docstring); at 8 pairs the text tower's do
    assert (_lib.GEMM_K_X3 in k_on) == (pairs * 77 > 512)
    if pairs * 77 > 512:
        assert not np.array_equal(on["txt_f"], off["txt_f"])      # the path changed the numbers: it really ran
        assert np.array_equal(on["img_f"], off["img_f"])          # the vision tower's forward is few-row throughout: untouched


@pytest.mark.parametrize("pairs", [4, 8])
def test_accuracy_against_the_f32_engine(pairs):
    r = runs(pairs)
    off, on, b16 = r["off"][0], r["on"][0], r["bf16"][0]
    groups = {"features": ("img_f", "txt_f", "enc_img", "enc_txt"), "logits": ("logits",), "losses": ("base_loss", "alignment_loss"), "factor gradients": GRADS}
    for name, keys in groups.items():
        e3 = max(maxerr(on[k], off[k]) for k in keys)
        eb = max(maxerr(b16[k], off[k]) for k in keys)
        print(f"gemm_bf16x3 tiny3 {pairs} pairs, {name}: e3 {e3:.3e}, e_bf16 {eb:.3e}" + (f" ({eb / e3:.0f} x)" if e3 > 0 else ""))
        assert e3 <= eb / 32.0, name
    for k in GRADS:
        a, b = on[k].astype(np.float64).ravel(), off[k].astype(np.float64).ravel()
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert cos >= MIN_GRAD_COSINE, (k, cos)


def _reference_errors(res, g):
    logit = maxerr(res["logits"], g["logits"])
    grad = max(maxerr(res[k], g[k]) / (float(np.abs(g[k]).max()) + 1e-30) for k in GRADS)
    return logit, grad


def _assert_measured(name, logit, grad):
    m = MEASURED[name]
    print(f"gemm_bf16x3 vs reference fixture {name}: max |logit - ref| {logit:.3e} (f32 bar 1e-4), factor-gradient max err / max |ref| {grad:.3e} (f32 bar 1e-3)")
    assert logit <= 2 * m["logits"]
    assert grad <= 2 * m["grads"]


def test_plugin_fused_step_on_tiny_d1(golden):
    """The plugin's fused step with engine_options {"gemm_bf16x3": true} against the reference-generated arrays of fixture tiny_d1."""
    from lpi_amd.retrieval.models.slinet import SliNet
    g = golden("tiny_d1")
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    args.update(backbonename="tiny", visual_dim=128, textual_dim=128, device=[torch.device(DEV)], compute_dtype="f32", batch_size=4, epochs=1, num_workers=0,
                engine_options={"gemm_bf16x3": True})
    net = SliNet(args).to(DEV)
    for t in range(len(net.prompts)):
        for k, v in synth.prompt_factors(9, 16, 128, 128, task=t).items():
            getattr(net.prompts[t], k).data = torch.from_numpy(v.copy()).to(DEV)
    net.numtask = 1
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad_("prompts.0." in n)
        p.grad = None
    out = net.train_step(torch.from_numpy(synth.images(4, 32)).to(DEV), torch.from_numpy(g["token_ids"]))
    torch.cuda.synchronize()
    assert net.engine.opt.gemm_bf16x3 is True
    res = {"logits": (net.engine.logit_scale_exp * out["image_features"].float() @ out["text_features"].float().t()).cpu().numpy()}
    for k in synth.PROMPT_NAMES:
        res["grad." + k] = getattr(net.prompts[0], k).grad.cpu().numpy()
    _assert_measured("tiny_d1", *_reference_errors(res, g))


def test_vitb16_d1_against_the_reference(golden):
    """ViT-B/16, 8 pairs, depth 1 (1 704 vision rows, 616 text rows: every full-block GEMM takes the bf16x3 kernels) against the reference-generated arrays."""
    cfg = synth.VIT_B16
    g = golden("vitb16_d1")
    enc = DualEncoder(cfg, synth.clip_state_dict(cfg), dtype="f32", device=DEV, options=EngineOptions(gemm_bf16x3=True))
    fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
    img = torch.from_numpy(synth.images(8, cfg.image_resolution)).to(DEV)
    E.GEMM_PROFILE = []
    try:
        out = train_step(enc, img, torch.from_numpy(g["token_ids"]).to(DEV), fac, 1)
        torch.cuda.synchronize()
        kinds = [p[4] for p in E.GEMM_PROFILE]
    finally:
        E.GEMM_PROFILE = None
    assert kinds.count(_lib.GEMM_K_X3) > len(kinds) // 2 and _lib.GEMM_K_ROWS in kinds
    res = {"logits": (enc.logit_scale_exp * out["img_f"] @ out["txt_f"].t()).cpu().numpy()}
    for k in synth.PROMPT_NAMES:
        res["grad." + k] = fac[k].grad.cpu().numpy()
    _assert_measured("vitb16_d1", *_reference_errors(res, g))
