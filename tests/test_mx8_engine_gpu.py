"""EngineOptions.mx8_forward on a real MI355X: the train=False forwards of both towers run their full blocks on the MX-FP8 kernels (and say so through
lpi_gemm_last_kernel), stay close to the f32 engine, leave the training step bit for bit alone, and carry the plugin's clustering and retrieval
evaluation."""
import json
import os

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
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# three layers: two full blocks per tower take the MX path, the pooled last block stays on the 2-byte kernels
TINY3 = ClipConfig("tiny3", 128, 32, 3, 128, 16, 77, 49408, 128, 2, 3)
# Measured on MI355X against the f32 engine on the same inputs: maximum absolute feature error 2.69e-2 / minimum per-sample cosine
# 0.99400 with the pooled last block, 2.64e-2 / 0.99288 with pooled_last=False (bf16 mode on the same inputs: 1.7e-3 / 0.99998; ViT-B/16: 9.8e-4).  The error
# bar is 2 x the measured maximum; the cosine bar is a condition, not a measurement: below 0.99 the mode is no use for retrieval.
FEATURE_BAR = {True: 2 * 2.69e-2, False: 2 * 2.64e-2}      # by pooled_last
MIN_COSINE = 0.99


def inputs(cfg, B=4):
    fac = {k: torch.from_numpy(v).to(DEV) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
    img = torch.from_numpy(synth.images(B, cfg.image_resolution)).to(DEV)
    ids = synth.token_ids(B)
    return fac, img, ids


def features(cfg, sd, dtype, img, ids, fac, depth=2, log=None, **opts):
    """(image features, text features) of the train=False encodes with prompts; text rows ragged (PackedIds), vision rows uniform."""
    enc = DualEncoder(cfg, sd, dtype=dtype, device=DEV, options=EngineOptions(**opts))
    with torch.no_grad():
        vis, txt = DecomposedPromptFn.apply(*[fac[k] for k in _CP_ORDER], 1.0, None)
    lib = _lib.load()
    if log is not None:      # a launch-kind log: which GEMM kernel every request of the towers launched
        issue = E.Mx8Req.issue

        def logged(self):
            issue(self)
            if self.name == "lpi_gemm_nt_mx8":
                log.append(int(lib.lpi_gemm_last_kernel()))
        E.Mx8Req.issue = logged
    try:
        fi = enc.encode_image(img, vis, depth, train=False)
        ft = enc.encode_text(PackedIds(ids).to(DEV), txt, depth, train=False)
        torch.cuda.synchronize()
    finally:
        if log is not None:
            E.Mx8Req.issue = issue
    return fi.float().cpu().numpy(), ft.float().cpu().numpy()


_CACHE = {}


def tiny3(pooled_last):
    """f32, bf16 and bf16 + mx8_forward features of the same inputs, computed once per arm."""
    if pooled_last not in _CACHE:
        cfg = TINY3
        sd = synth.clip_state_dict(cfg)
        fac, img, ids = inputs(cfg)
        log = []
        _CACHE[pooled_last] = {
            "f32": features(cfg, sd, "f32", img, ids, fac, pooled_last=pooled_last),
            "bf16": features(cfg, sd, "bf16", img, ids, fac, pooled_last=pooled_last),
            "mx8": features(cfg, sd, "bf16", img, ids, fac, log=log, pooled_last=pooled_last, mx8_forward=True),
            "log": log,
        }
    return _CACHE[pooled_last]


def err_and_cos(got, ref):
    err = max(float(np.abs(g - r).max()) for g, r in zip(got, ref))
    cos = min(float(((g * r).sum(1) / (np.linalg.norm(g, axis=1) * np.linalg.norm(r, axis=1))).min()) for g, r in zip(got, ref))
    return err, cos


@pytest.mark.parametrize("pooled_last", [True, False])
def test_tiny_towers(pooled_last):
    r = tiny3(pooled_last)
    full = 2 if pooled_last else 3
    # four MX GEMMs per full block per tower, each attributed to the MX kernel
    assert r["log"] == [_lib.GEMM_K_MX8] * (2 * full * 4)
    # not the bf16 engine's numbers: the path really ran
    assert any(np.abs(a - b).max() > 0 for a, b in zip(r["mx8"], r["bf16"]))
    err, cos = err_and_cos(r["mx8"], r["f32"])
    err16, cos16 = err_and_cos(r["bf16"], r["f32"])
    print(f"mx8_forward tiny3 pooled_last={pooled_last}: max |feature - f32| {err:.3e} (bf16 mode {err16:.3e}), min cosine {cos:.6f} (bf16 mode {cos16:.6f})")
    assert cos >= MIN_COSINE
    assert err <= FEATURE_BAR[pooled_last]


def test_train_step_is_bitwise_unchanged():
    cfg = synth.TINY
    sd = synth.clip_state_dict(cfg)
    ids = synth.token_ids(4)
    img = torch.from_numpy(synth.images(4, cfg.image_resolution)).to(DEV)
    outs = []
    for on in (False, True):
        enc = DualEncoder(cfg, sd, dtype="bf16", device=DEV, options=EngineOptions(mx8_forward=on))
        fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
        if on:      # a no-grad forward first: its MX buffers and launches must leave the training arena alone
            enc.encode_image(img, None, 1, train=False)
        out = train_step(enc, img, PackedIds(ids, 17).to(DEV), fac, 2)
        torch.cuda.synchronize()
        outs.append({**{k: out[k].detach().cpu() for k in ("img_f", "txt_f", "base_loss", "alignment_loss")},
                     **{"grad." + k: fac[k].grad.cpu() for k in synth.PROMPT_NAMES}})
    assert set(outs[0]) == set(outs[1]) and len(outs[0]) == 9
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_workspace_unchanged_with_the_option_off_and_refused_in_f32():
    cfg = synth.TINY
    sd = synth.clip_state_dict(cfg)
    off = DualEncoder(cfg, sd, dtype="bf16", device=DEV)
    on = DualEncoder(cfg, sd, dtype="bf16", device=DEV, options=EngineOptions(mx8_forward=True))
    size = lambda ws: {k: (tuple(v.shape), v.dtype) for k, v in ws.items() if torch.is_tensor(v)}  # noqa: E731
    for train in (False, True):
        a, b = off.vis.workspace(4, 21, train), on.vis.workspace(4, 21, train)
        assert size(a) == size(b)
        assert ("mx" in b) == (not train) and "mx" not in a
    assert not hasattr(off.vis.blocks[0]["qkv"], "w8") and on.vis.blocks[0]["qkv"].w8.dtype == torch.uint8
    with pytest.raises(ValueError):
        DualEncoder(cfg, sd, dtype="f32", device=DEV, options=EngineOptions(mx8_forward=True))


def test_plugin_clustering_and_retrieval():
    from lpi_amd.retrieval.utils import factory
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    args.update(backbonename="tiny", visual_dim=128, textual_dim=128, device=[torch.device(DEV)], compute_dtype="bf16", batch_size=4, epochs=1, num_workers=0,
                dataset_impl="synthetic", synthetic_train_size=16, synthetic_eval_images_per_task=12)
    runs = []
    for eo in (None, {"mx8_forward": True}):
        a = dict(args)
        if eo is not None:
            a["engine_options"] = eo
        m = factory.get_model("sprompts", a)
        net = m._network.to(DEV)
        for t in range(len(net.prompts)):
            for k, v in synth.prompt_factors(9, 16, 128, 128, task=t).items():
                getattr(net.prompts[t], k).data = torch.from_numpy(v.copy()).to(DEV)
        net.numtask = 1
        m.cur_id = 0
        train_ds, test_ds = m._datasets(0)
        train_loader, test_loader = m._loaders(train_ds, test_ds)
        n0 = _lib.launch_count()
        m.clustering(train_loader)
        s_i2t, s_t2i, res = m._evaluate_retrieval(test_loader)
        assert _lib.launch_count() > n0
        assert net.engine.opt.mx8_forward is bool(eo)
        assert len(m.all_keys) == 1 and m.all_keys[0].shape == (5, 128) and m.textual_all_keys[0].shape == (5, 128)
        assert set(res) == {"mscoco"} and set(res["mscoco"]) == {"i2t", "t2i"} and set(res["mscoco"]["i2t"]) == {0}
        assert all(len(v) == 3 and 0 <= v[0] <= v[1] <= v[2] <= 100 for v in res["mscoco"]["t2i"].values())
        runs.append((s_i2t, s_t2i))
    # top-1 agrees with the option-off run wherever its margin between rank 1 and rank 2 exceeds twice the measured error of the scores (the rule of
    # tests/test_reference_bs256_gpu.py, which measures the logits).  The features of a random-weight backbone lie close together: few queries are decidable
    # (measured: 1 of 36 at a score error of 1.2e-2), so the count is printed, not asserted.
    checked = 0
    for off, on in zip(runs[0], runs[1]):
        err = float(np.abs(on - off).max())
        top = np.sort(off, axis=1)
        safe = (top[:, -1] - top[:, -2]) > 2 * err
        assert (np.argmax(on, axis=1)[safe] == np.argmax(off, axis=1)[safe]).all()
        checked += int(safe.sum())
        print(f"mx8_forward plugin: score error {err:.3e}, {int(safe.sum())} of {len(safe)} queries decidable")
    assert not np.array_equal(runs[0][0], runs[1][0])      # the option changed the features: the path ran
