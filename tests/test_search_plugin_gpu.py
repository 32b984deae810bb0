"""eval_scores = 'streamed' through the plugin at ViT-B/16 size: SPrompts._evaluate_retrieval in both modes on one object, built as
tests/test_fullsize_gpu.py::test_eval_shard_at_vitb16_size_matches_reference builds it, against the reference-generated fixture."""
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


@pytest.mark.parametrize("name", ["vitb16_eval", "vitb16_eval12"])
def test_streamed_evaluation_matches_matrix_mode_and_fixture(golden, name, monkeypatch):
    """Streamed mode returns (None, None, res).  Every R@K per task may differ from the fixture's only by the undecided rows of the reference's own
    test, with err = the matrix mode's measured score error against the fixture + E * 2^-24 (the streamed scores are not returned, so their distance from
    the fixture is bounded by the matrix mode's plus the worst-case difference of two f32 dot products of unit vectors' f64 value).  The ranks gt_rank
    gave inside the plugin equal lpi_retrieval_rank on the matrix mode's scores wherever the fixture's margin exceeds 10 err."""
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    g = golden(name)
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

    s_i2t, s_t2i, res_matrix = m._evaluate_retrieval(Loader())
    assert s_i2t.shape == (n_img, n_txt) and s_t2i.shape == (n_txt, n_img)

    calls = []
    real = search.gt_rank

    def recording(q, gal, gt):
        r = real(q, gal, gt)
        calls.append((tuple(q.shape), tuple(gal.shape), r.cpu().numpy().astype(np.int64)))
        return r

    monkeypatch.setattr(search, "gt_rank", recording)
    m.args["eval_scores"] = "streamed"
    out = m._evaluate_retrieval(Loader())
    m.args["eval_scores"] = "matrix"
    assert out[0] is None and out[1] is None
    res = out[2]
    E = CFG.embed_dim
    assert [c[:2] for c in calls] == [((n_img, E), (n_txt, E)), ((n_txt, E), (n_img, E))]

    err_matrix = float(np.abs(s_i2t - g["score_i2t"]).max())
    err = err_matrix + E * 2.0 ** -24
    s = torch.cuda.current_stream().cuda_stream
    for S, gts, ref_r, ref_m, tag, got in ((s_i2t, [DS.img2txt[i] for i in range(n_img)], g["rank_i2t"], g["rank_margin_i2t"], "i2t", calls[0][2]),
                                           (s_t2i, [[DS.txt2img[t]] for t in range(n_txt)], g["rank_t2i"], g["rank_margin_t2i"], "t2i", calls[1][2])):
        gt = torch.tensor(gts, dtype=torch.int32, device=DEV)
        r = torch.zeros(len(gts), dtype=torch.int32, device=DEV)
        Sd = torch.from_numpy(np.ascontiguousarray(S)).to(DEV)
        _lib.call("lpi_retrieval_rank", Sd.shape[0], Sd.shape[1], Sd, Sd.shape[1], gt, gt.shape[1], r, s)
        of_matrix = r.cpu().numpy().astype(np.int64)
        safe = ref_m > 10 * err
        print(f"{name} {tag}: matrix-mode score error {err_matrix:.2e}, err {err:.2e}; streamed ranks equal the matrix mode's on "
              f"{int((got == of_matrix).sum())} of {len(safe)} rows, asserted on {int(safe.sum())}")
        assert np.array_equal(got[safe], of_matrix[safe])
        Sref = g["score_i2t"] if tag == "i2t" else g["score_i2t"].T
        close = np.array([max(int((np.abs(Sref[i] - Sref[i, j]) <= 2 * err).sum()) - 1 for j in gts[i]) for i in range(len(gts))])
        cat = g["cat_i"] if tag == "i2t" else g["cat_t"]
        for t in range(n_tasks):
            rows = cat == t
            for ki, kk in enumerate((1, 5, 10)):
                undecided = int(((ref_r[rows] - close[rows] < kk) & (ref_r[rows] + close[rows] >= kk)).sum())
                refv = g["itm_" + tag][t][ki]
                assert abs(res["mscoco"][tag][t][ki] - refv) <= 100.0 * undecided / max(1, int(rows.sum())) + 1e-9, (tag, t, kk)
    assert set(res["mscoco"]) == set(res_matrix["mscoco"]) and set(res["mscoco"]["i2t"]) == set(res_matrix["mscoco"]["i2t"])
