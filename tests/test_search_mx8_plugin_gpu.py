"""eval_search_operands = 'mx8' through the plugin at ViT-B/16 size: SPrompts._evaluate_retrieval in streamed mode on one object, built as
tests/test_search16_plugin_gpu.py builds it."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lpi_amd import _lib, search, synth  # noqa: E402

DEV = "cuda:0"
CFG = synth.VIT_B16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_streamed_evaluation_with_mx8_search_operands(golden, monkeypatch):
    """With eval_search_operands = 'mx8' both gt_rank calls carry operands="mx8", the image and the text features are quantised exactly once each
    (quantize_mx8 runs twice, and gt_rank receives Mx8Rows), and the recorded ranks EQUAL lpi_search_rank_mx8 called directly on quantize_mx8 of the same
    features (integers: the equality is exact).  With the key absent, and with 'f32', the evaluation is what it is without this operand type.

    R@K is printed beside the fixture's values and nothing is asserted against the fixture: the rigorous bound on the change of a score when two unit
    vectors are rounded to MX-FP8 is 2u + u^2 with u = 2^-4 + sqrt(32) 2^-17.8 ~ 0.063 (relative rounding of an e4m3 element, plus the absolute rounding
    of the elements of a block in the subnormal range of its scale), about 0.13, which exceeds every margin of this fixture (32 images x 64 captions,
    synthetic weights): such an assertion would decide no row.  The kernels' own exactness is tests/test_search_mx8_gpu.py's."""
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    g = golden("vitb16_eval")
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    args.update(device=[torch.device(DEV)], compute_dtype="f32", num_workers=0, trim_text=True)
    m = SPrompts(args)
    net = m._network.to(torch.device(DEV))
    for t in range(len(net.prompts)):
        for k, v in synth.prompt_factors(9, 16, CFG.vision_width, CFG.transformer_width, task=t).items():
            getattr(net.prompts[t], k).data = torch.from_numpy(v.copy()).to(DEV)
    n_tasks, cpi = int(g["n_tasks"]), int(g["caps_per_img"])
    net.numtask = n_tasks
    m.cur_id = n_tasks - 1
    m.all_keys = [torch.from_numpy(k).to(DEV) for k in g["vkeys"]]
    m.textual_all_keys = [torch.from_numpy(k).to(DEV) for k in g["tkeys"]]
    n_img, n_txt = g["score_i2t"].shape
    img = torch.from_numpy(synth.images(n_img, 224, seed=synth.IMAGE_SEED + 11))

    class DS:
        text = torch.from_numpy(g["token_ids"].astype(np.int64))
        text_cat = list(g["cat_t"])
        img2txt = {i: [cpi * i + j for j in range(cpi)] for i in range(n_img)}
        txt2img = {t: t // cpi for t in range(n_txt)}

    class Loader:
        dataset = DS()

        def __iter__(self):
            for i in range(0, n_img, 16):
                yield img[i:i + 16], torch.arange(i, min(n_img, i + 16)), torch.from_numpy(g["cat_i"][i:i + 16])

    calls, quantised = [], []
    real_rank, real_quant = search.gt_rank, search.quantize_mx8

    def recording(q, gal, gt, **kw):
        r = real_rank(q, gal, gt, **kw)
        calls.append((kw.get("operands"), r.cpu().numpy().astype(np.int64), q, gal, gt))
        return r

    def quantising(x):
        quantised.append(x)
        return real_quant(x)

    monkeypatch.setattr(search, "gt_rank", recording)
    monkeypatch.setattr(search, "quantize_mx8", quantising)      # gt_rank's own quantisation of a float operand goes through this name too

    def streamed(ops):
        m.args["eval_scores"] = "streamed"
        if ops is not None:
            m.args["eval_search_operands"] = ops
        del calls[:], quantised[:]
        try:
            out = m._evaluate_retrieval(Loader())
        finally:
            m.args["eval_scores"] = "matrix"
            m.args.pop("eval_search_operands", None)
        assert out[0] is None and out[1] is None and len(calls) == 2
        return out[2], list(calls), len(quantised)

    res_absent, seen, nquant = streamed(None)
    assert [c[0] for c in seen] == [None, None] and nquant == 0
    ranks_absent = [c[1] for c in seen]
    res_f32, seen, nquant = streamed("f32")
    assert [c[0] for c in seen] == [None, None] and nquant == 0      # 'f32' is the call as it was: gt_rank's default
    assert res_f32 == res_absent and all(np.array_equal(a, b[1]) for a, b in zip(ranks_absent, seen))

    res, seen, nquant = streamed("mx8")
    assert [c[0] for c in seen] == ["mx8", "mx8"]
    assert nquant == 2      # image and text features once each, reused in both directions
    (_, r_i, q_i, g_i, gt_i), (_, r_t, q_t, g_t, gt_t) = seen
    assert all(isinstance(x, search.Mx8Rows) for x in (q_i, g_i, q_t, g_t)) and q_i is g_t and g_i is q_t
    image_f, text_f = quantised      # the features the plugin quantised
    assert tuple(image_f.shape) == (n_img, CFG.embed_dim) and tuple(text_f.shape) == (n_txt, CFG.embed_dim)
    s = torch.cuda.current_stream().cuda_stream
    for tag, qf, gf, gt, got in (("i2t", image_f, text_f, gt_i, r_i), ("t2i", text_f, image_f, gt_t, r_t)):
        q8, g8 = real_quant(qf), real_quant(gf)
        gt = torch.as_tensor(gt).to(device=DEV, dtype=torch.int32).reshape(q8.shape[0], -1).contiguous()
        n = int(_lib.load().lpi_search_workspace(q8.shape[0], g8.shape[0], 0))
        ws = torch.empty(n, dtype=torch.uint8, device=DEV)
        rank = torch.empty(q8.shape[0], dtype=torch.int32, device=DEV)
        _lib.call("lpi_search_rank_mx8", q8.shape[0], g8.shape[0], CFG.embed_dim, q8.codes, q8.codes.stride(0), q8.scales, q8.scales.stride(0),
                  g8.codes, g8.codes.stride(0), g8.scales, g8.scales.stride(0), gt, gt.shape[1], rank, ws, n, s)
        assert np.array_equal(rank.cpu().numpy().astype(np.int64), got), tag
        print(f"mx8 {tag}: ranks equal the f32 streamed search's on {int((got == ranks_absent[0 if tag == 'i2t' else 1]).sum())} of {len(got)} rows")
        for t in range(n_tasks):
            for ki, kk in enumerate((1, 5, 10)):
                print(f"mx8 {tag} task {t} R@{kk}: {res['mscoco'][tag][t][ki]:.2f} (fixture {g['itm_' + tag][t][ki]:.2f}, f32 streamed "
                      f"{res_absent['mscoco'][tag][t][ki]:.2f})")
