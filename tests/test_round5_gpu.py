"""Round-5 additions on a real MI355X:
  * the FUSED plugin step (SliNet.train_step: what SPrompts.train_epoch runs) against the reference's fixtures — losses and factor gradients, with and
    without the task term of a continual session (tiny_d1 / tiny_task2), and against the reference-ordered loop (net -> cal_loss -> backward);
  * the input pipeline (lpi_amd/pipeline.py): batches arrive bit for bit, in order, over several epochs, with a ragged last batch; a loader error
    reaches the consumer; an early exit stops the producer;
  * the plugin's hot loop on caption STRINGS and HOST images at the benchmarked size issues exactly the launches of the bare step and no other kernel;
  * a CLIP checkpoint file (TorchScript archive / saved state dict, fp16) gives the same features, bit for bit, as the in-memory state dict."""
import json
import os
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lpi_amd import _lib, synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RET = os.path.join(REPO, "lpi_amd", "retrieval")
DEV = torch.device("cuda:0")


def tiny_args(**over):
    args = json.load(open(os.path.join(RET, "configs", "lpi", "coco_lpi.json")))
    args.update(backbonename="tiny", visual_dim=128, textual_dim=128, device=[DEV], compute_dtype="f32", batch_size=4, epochs=1, num_workers=0)
    args.update(over)
    return args


def set_factors(net):
    for t in range(len(net.prompts)):
        for k, v in synth.prompt_factors(9, 16, 128, 128, task=t).items():
            getattr(net.prompts[t], k).data = torch.from_numpy(v.copy()).to(DEV)


# ------------------------------------------------------------------------------------------------ fused step vs the reference's fixtures
@pytest.mark.parametrize("name,numtask", [("tiny_d1", 1), ("tiny_task2", 2)])
def test_fused_plugin_step_matches_reference(golden, name, numtask):
    from lpi_amd.retrieval.models.slinet import SliNet
    g = golden(name)
    net = SliNet(tiny_args()).to(DEV)
    set_factors(net)
    net.numtask = numtask
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad_("prompts." + str(numtask - 1) + "." in n)
        p.grad = None
    img = torch.from_numpy(synth.images(4, 32)).to(DEV)
    n0 = _lib.launch_count()
    out = net.train_step(img, torch.from_numpy(g["token_ids"]))
    torch.cuda.synchronize()
    assert _lib.launch_count() - n0 > 30
    assert np.abs(out["image_features"].cpu().numpy() - g["img_f"]).max() < 1e-4
    assert np.abs(out["text_features"].cpu().numpy() - g["txt_f"]).max() < 1e-4
    losses = out["loss"]
    assert set(losses) == ({"base_loss", "alignment_loss"} | ({"task_loss"} if numtask != 1 else set()))
    for k, v in losses.items():
        got = sum(float(p) for p in v) if isinstance(v, tuple) else float(v)
        assert abs(got - float(g[k])) < 1e-4 * max(1.0, abs(float(g[k]))), (k, got, float(g[k]))
    for k in synth.PROMPT_NAMES:
        got = getattr(net.prompts[numtask - 1], k).grad.cpu().numpy()
        ref = g["grad." + k]
        assert np.abs(got - ref).max() <= 1e-3 * np.abs(ref).max() + 1e-5, k
    # a second step on the same network: the task term's cached rows / the seeded buffers carry nothing over (same inputs, same gradients)
    g1 = {k: getattr(net.prompts[numtask - 1], k).grad.clone() for k in synth.PROMPT_NAMES}
    net.train_step(img, torch.from_numpy(g["token_ids"]))
    for k in synth.PROMPT_NAMES:
        assert torch.equal(getattr(net.prompts[numtask - 1], k).grad, g1[k]), k


@pytest.mark.parametrize("numtask", [1, 2])
def test_pipelined_fused_loop_equals_the_reference_ordered_loop(numtask, monkeypatch):
    """SPrompts._train three epochs of two batches: (pipeline + fused step + FlatSGD) and (images.to(device) -> net -> cal_loss -> sum -> backward ->
    FlatSGD, the reference's order) move the parameters to the same place (same kernels for forward / backward; the fused path only skips the scalar loss
    graph: one multiplication by 1.0 less per gradient)."""
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    ids = torch.from_numpy(synth.token_ids(8, seed=5))
    img = torch.from_numpy(synth.images(8, 32, seed=11))
    loader = [(img[:4], ids[:4], 0, 0), (img[4:], ids[4:], 0, 0)]
    got = []
    for fast in (True, False):
        m = SPrompts(tiny_args(epochs=3, prefetch=fast, fused_step=fast))
        net = m._network.to(DEV)
        set_factors(net)
        net.numtask = numtask
        monkeypatch.setattr(m, "clustering", lambda dataloader: None)
        monkeypatch.setattr(m, "_evaluate_retrieval", lambda loader: (None, None, {}))
        m._train(loader, None)
        torch.cuda.synchronize()
        got.append({k: getattr(net.prompts[numtask - 1], k).detach().clone() for k in synth.PROMPT_NAMES})
    for k in synth.PROMPT_NAMES:
        start = torch.from_numpy(synth.prompt_factors(9, 16, 128, 128, task=numtask - 1)[k]).to(DEV)
        moved = float((got[1][k] - start).abs().max())
        assert moved > 0
        assert float((got[0][k] - got[1][k]).abs().max()) <= 1e-5 * moved + 1e-7, k


# ------------------------------------------------------------------------------------------------ input pipeline
def test_pipeline_batches_arrive_bit_for_bit_in_order_over_epochs():
    from lpi_amd.engine import PackedIds
    from lpi_amd.pipeline import BatchPipeline
    g = torch.Generator().manual_seed(3)
    n, B = 22, 4                                   # 5 full batches and a ragged last one of 2
    imgs = torch.randn(n, 3, 32, 32, generator=g)
    ids = torch.from_numpy(synth.token_ids(n, seed=9))
    # three loader flavours: a stacked tensor, a list of per-item views (collate_keep_images), a non-contiguous stacked tensor
    loaders = [[(imgs[i:i + B], ids[i:i + B], 0, 7) for i in range(0, n, B)],
               [([imgs[j] for j in range(i, min(n, i + B))], ids[i:i + B], 0, 7) for i in range(0, n, B)],
               [(imgs[i:i + B].transpose(2, 3).contiguous().transpose(2, 3), ids[i:i + B], 0, 7) for i in range(0, n, B)]]
    for loader in loaders:
        pipe = BatchPipeline(loader, DEV, lambda c: PackedIds(c), depth=2, threads=3, timing=True)
        for epoch in range(3):
            seen = 0
            for b in pipe:
                lo = b.index * B
                hi = min(n, lo + B)
                assert b.images.shape == (hi - lo, 3, 32, 32) and b.images.is_cuda
                # consume on the CURRENT stream, like the step does (the pipeline made it wait for the copy)
                assert torch.equal(b.images.cpu(), imgs[lo:hi])
                assert isinstance(b.text, PackedIds) and torch.equal(b.text._dev.cpu(), PackedIds(ids[lo:hi]).ids)
                assert b.rest == (0, 7) and set(b.host_ms) >= {"gather", "tokenise_pack"}
                assert b.h2d[0].elapsed_time(b.h2d[1]) >= 0.0 if epoch else True
                seen += 1
            assert seen == 6
    assert not pipe._thread.is_alive()


def test_pipeline_passes_loader_errors_on_and_stops_on_early_exit():
    from lpi_amd.pipeline import BatchPipeline

    def bad():
        yield torch.zeros(2, 3, 8, 8), torch.zeros(2, 77, dtype=torch.long)
        raise OSError("disk gone")
    got = 0
    with pytest.raises(OSError, match="disk gone"):
        for b in BatchPipeline(bad(), DEV, None):
            got += 1
    assert got == 1
    many = [(torch.zeros(2, 3, 8, 8), torch.zeros(2, 77, dtype=torch.long)) for _ in range(50)]
    pipe = BatchPipeline(many, DEV, None, depth=2)
    it = iter(pipe)
    b0 = next(it)
    assert pipe._done[b0.slot] is None
    it.close()                                     # the consumer leaves after one batch
    # the batch that was out when the pass ended has its end-of-use event, so the next pass (slot indices restart at 0) cannot copy into
    # a ring slot that a step in flight still reads
    assert pipe._done[b0.slot] is not None
    pipe._thread.join(timeout=5.0)
    assert not pipe._thread.is_alive()
    assert not [t for t in threading.enumerate() if t.name == "lpi-batch-pipeline" and t.is_alive()]


# ------------------------------------------------------------------------------------------------ the plugin's hot loop at the benchmarked size
def test_plugin_loop_on_strings_issues_the_bare_steps_launches_and_no_other_kernel(tmp_path, monkeypatch):
    """SPrompts.train_epoch over a DataLoader of HOST f32 images and caption STRINGS (ViT-B/16, 256 pairs, bf16, depth 3): per iteration exactly the
    library launches of the bare step (lpi_amd.step.train_step + FlatSGD on resident tensors: 217 in the plain packed text layout, tests/test_round4_gpu.py,
    + 13 in the shared-prefix layout the plugin trains on: one lpi_shared_kv_reduce per text block, and the first block's prompt-row dgrad GEMMs no longer
    pair — the text tower's has 16 rows) and NO other device
    kernel — the H2D copies are DMA (Memcpy), the tokenizer is host code, the loss log holds references."""
    from torch.profiler import ProfilerActivity, profile
    from torch.utils.data import DataLoader
    from lpi_amd import synth_bpe
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    from lpi_amd.retrieval.models.clip import prompt_learner as PL
    from lpi_amd.retrieval.utils.data import SyntheticCoco, collate_keep_images
    monkeypatch.setenv("LPI_BPE_VOCAB", synth_bpe.write_table(tmp_path / "bpe.txt.gz", seed=1))
    monkeypatch.setattr(PL, "_tokenizer", None)
    B = 256
    args = json.load(open(os.path.join(RET, "configs", "lpi", "coco_lpi.json")))
    args.update(device=[DEV], compute_dtype="bf16", honor_prompt_depth=True, prompt_depth=3, batch_size=B, epochs=1, num_workers=0)
    m = SPrompts(args)
    net = m._network
    net.update_fc(0)
    ds = SyntheticCoco(12 * B, [0], 224, captions="strings", image_pool=64)
    loader = DataLoader(ds, batch_size=B, shuffle=False, num_workers=0, collate_fn=collate_keep_images)
    opt, _ = m._setup_training()
    counts = []
    prof = profile(activities=[ProfilerActivity.CUDA])
    state = {"profile": False}

    def on_step(i, batch, out):
        counts.append(_lib.launch_count())
        if state["profile"] and i == 2:            # exactly ONE iteration of the running loop under the profiler: iteration 3
            torch.cuda.synchronize()
            prof.start()
        if state["profile"] and i == 3:
            torch.cuda.synchronize()
            prof.stop()
        return i == 5
    m.train_epoch(loader, opt, 0, None, on_step)            # warm-up pass: arenas, pinned slots, tokenizer tables
    torch.cuda.synchronize()
    state["profile"] = True
    dev_events = []
    for attempt in range(8):      # the tracer now and then hands back a fraction of a window's records (17 of 237, 28 of 230 three times running): profile another pass then
        counts.clear()
        prof = profile(activities=[ProfilerActivity.CUDA])
        m.train_epoch(loader, opt, 0, None, on_step)
        torch.cuda.synchronize()
        dev_events = [e.name for e in prof.events() if e.device_type.name != "CPU"]
        if len(dev_events) >= 200:
            break
    per = sorted({b - a for a, b in zip(counts, counts[1:])})
    print(f"\n    library launches per iteration of the plugin loop: {per}")
    # the bare step on resident tensors of the same batch
    from lpi_amd.step import train_step
    img = torch.stack([ds[i][0] for i in range(B)]).to(DEV)
    pk = net.prepare_text([ds[i][1] for i in range(B)]).to(DEV)
    fac = net.task_factors()
    for _ in range(2):
        n0 = _lib.launch_count()
        train_step(net.engine, img, pk, fac, 3, flat_grad=opt.flat_grad, grad_views=opt.grad_views)
        opt.step()
        bare = _lib.launch_count() - n0
    assert pk.shared == 17
    assert len(per) == 1 and per[0] == bare and bare <= 232, (per, bare)      # 237 + 6 - 13 = 230 since round 6 (the last block without K and V, the few-row GEMMs in one launch: tests/test_round4_gpu.py)
    from lpi_amd import engine as E
    # no request without its partner in this configuration (towers of equal depth): counted over the bare steps above
    stats0 = dict(E.LOCKSTEP_STATS)
    train_step(net.engine, img, pk, fac, 3, flat_grad=opt.flat_grad, grad_views=opt.grad_views)
    assert E.LOCKSTEP_STATS["paired"] > stats0["paired"] and E.LOCKSTEP_STATS["shifted"] == stats0["shifted"], (stats0, E.LOCKSTEP_STATS)
    foreign = [n for n in dev_events if "anonymous namespace" not in n and "_GLOBAL__N_" not in n and "lpi" not in n.lower() and "StatFin" not in n
               and "Memcpy" not in n and "Memset" not in n]
    assert len(dev_events) >= bare and foreign == [], (len(dev_events), sorted(set(foreign)))
    monkeypatch.setattr(PL, "_tokenizer", None)


# ------------------------------------------------------------------------------------------------ checkpoint files
def test_features_from_a_checkpoint_file_equal_those_from_the_state_dict(tmp_path):
    """args['clip_state_dict'] = <path>: a TorchScript archive (how OpenAI ships CLIP; torch.jit.load(...).state_dict(), prompt_learner.py:15-17) and a
    torch.save'd fp16 state dict with the three scalar entries build_model drops — the engine built from either gives the features of the engine built
    from the in-memory dict, bit for bit; the architecture comes from the tensor shapes."""
    from lpi_amd.checkpoint import ParamTree
    from lpi_amd.retrieval.models.slinet import SliNet
    cfg = synth.TINY
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in synth.clip_state_dict(cfg).items()}
    half = {k: (v.half() if v.is_floating_point() else v) for k, v in sd.items()}
    half.update(input_resolution=torch.tensor(32), context_length=torch.tensor(77), vocab_size=torch.tensor(49408))
    p_dict, p_jit = str(tmp_path / "clip_sd.pt"), str(tmp_path / "clip_jit.pt")
    torch.save(half, p_dict)
    torch.jit.save(torch.jit.script(ParamTree(half)), p_jit)
    img = torch.from_numpy(synth.images(4, 32)).to(DEV)
    ids = torch.from_numpy(synth.token_ids(4))
    feats = []
    for src in ({k: v.float() for k, v in half.items() if v.is_floating_point()}, p_dict, p_jit):
        net = SliNet(tiny_args(clip_state_dict=src, compute_dtype="f16")).to(DEV)
        set_factors(net)
        net.numtask = 1
        net.eval()
        assert net.clip_cfg.as_clip_args() == cfg.as_clip_args()
        with torch.no_grad():
            fi, ft, _, _ = net(img, ids)
        feats.append((fi.clone(), ft.clone()))
    for fi, ft in feats[1:]:
        assert torch.equal(fi, feats[0][0]) and torch.equal(ft, feats[0][1])
    # fp16 weights are exactly representable in every operand type of the f16 mode: the f32 original of the same weights gives the same features
    # wherever the engine rounds to fp16 anyway — checked against the widened copy above, not against the unrounded f32 weights
    with pytest.raises(ValueError):
        SliNet(tiny_args(clip_state_dict=p_dict, backbonename="tiny14", visual_dim=256))


# ------------------------------------------------------------------------------------------------ one-sweep LayerNorm statistics: the guard
def _hostile_weights(cfg):
    """ViT-B/16 synthetic weights with the two things real CLIP residual streams are known for and N(0, sigma) weights lack: rows whose MEAN is tens of
    deviations out (a uniform +40 on a vision block's c_proj bias: LayerNorm removes it exactly, E[x^2] - mean^2 does not) and 'massive activation'
    channels (two text channels pushed hundreds of deviations out: large variance, harmless to the one-sweep form)."""
    sd = {k: np.array(v, copy=True) for k, v in synth.clip_state_dict(cfg).items()}
    sd["visual.transformer.resblocks.2.mlp.c_proj.bias"] = sd["visual.transformer.resblocks.2.mlp.c_proj.bias"] + np.float32(40.0)
    b = sd["transformer.resblocks.1.mlp.c_proj.bias"]
    b[5] += 300.0
    b[400] -= 180.0
    return sd


def test_one_sweep_statistics_guard_switches_to_the_statistics_pass(monkeypatch):
    """Full ViT-B/16, bf16 mode, weights that put every vision row at |mean| >= 20 std from block 3 on.  The guard counts those rows in the first forward
    (no synchronisation: the verdict is read when its copy has landed), warns, and the next forward runs the two-sweep statistics pass: its features are
    exact to f32 round-off where the one-sweep ones were wrong in the fourth digit.  (At the FEATURE level the two are indistinguishable: see the
    comment at the assertion.)"""
    from lpi_amd import engine as E
    from lpi_amd.engine import DualEncoder, PackedIds
    cfg = synth.CONFIGS["ViT-B/16"]
    sd = _hostile_weights(cfg)
    Bq = 32
    img = torch.from_numpy(synth.images(Bq, 224)).to(DEV)
    ids = synth.token_ids(Bq)
    fac = synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width)
    from lpi_amd.functional import DecomposedPromptFn
    vis, txt = DecomposedPromptFn.apply(*[torch.from_numpy(fac[k]).to(DEV) for k in synth.PROMPT_NAMES])

    def feats(enc):
        with torch.no_grad():
            (fi, _), (ft, _) = enc.encode_both(img, PackedIds(ids).to(DEV), vis, txt, 3, train=False)
        torch.cuda.synchronize()
        return fi.clone(), ft.clone()
    enc32 = DualEncoder(cfg, sd, dtype="f32", device=DEV)
    ri, rt = feats(enc32)
    del enc32
    err = lambda f: (float((f[0] - ri).abs().max()), float((f[1] - rt).abs().max()))  # noqa: E731

    def rstd_err(enc):
        """worst relative error of the ln_1 rstd the vision tower USED in blocks 4.., against two-pass f64 statistics of the stored fp16 stream rows"""
        with torch.no_grad():
            (_, cv), _ = enc.encode_both(img, PackedIds(ids).to(DEV), vis, txt, 3, train=True)
        torch.cuda.synchronize()
        ws, worst, ratio = cv[0], 0.0, 0.0
        for i in range(4, 11):
            x = ws["x"][i][:ws["M"]].double()
            ref = 1.0 / (x.var(1, unbiased=False) + 1e-5).sqrt()
            worst = max(worst, float((ws["stat"][i][1][:ws["M"]].double() / ref - 1).abs().max()))
            ratio = max(ratio, float((x.mean(1).abs() / x.std(1, unbiased=False)).max()))
        return worst, ratio
    enc = DualEncoder(cfg, sd, dtype="bf16", device=DEV)
    assert enc.vis.rowstats == 2 and enc.txt.rowstats == 2
    first = err(feats(enc))                      # one-sweep statistics: the guard counts, nothing has switched yet
    assert enc.rowstat_guard_tripped == 0
    with pytest.warns(RuntimeWarning, match="two-sweep statistics pass"):
        second = err(feats(enc))                 # the verdict has landed: this forward runs the statistics pass
    assert enc.rowstat_guard_tripped > 0 and enc.vis.rowstats == 0 and enc.txt.rowstats == 0
    third = err(feats(enc))
    assert third == second                       # stays switched, deterministic
    guarded_stat, ratio = rstd_err(enc)
    enc0 = DualEncoder(cfg, sd, dtype="bf16", device=DEV, options=E.EngineOptions(rowstat_guard=False))
    unguarded = [err(feats(enc0)) for _ in range(2)][-1]
    unguarded_stat, _ = rstd_err(enc0)
    assert enc0.vis.rowstats == 2 and enc0.rowstat_guard_tripped == 0
    print(f"\n    rows at |mean| / std up to {ratio:.0f}: rstd relative error one-sweep {unguarded_stat:.2e}, after the switch {guarded_stat:.2e};"
          f" max |feature - f32 HIP| (image, text): one-sweep {first}, after the switch {second}, guard off {unguarded}")
    # the statistics: wrong in the fourth digit without the switch, exact to f32 round-off with it
    assert ratio >= 30 and unguarded_stat > 1e-4 and guarded_stat < 2e-6
    # the features: at these rows the fp16 residual stream's own rounding (the reference's activation type, 11 bits on a mean 40 deviations out) is what
    # separates the mode from the f32 path — measured 5.7e-3 with either statistics (tools/rowstat_guard_probe.py; profiles/r05_rowstat_guard.md: the same up
    # to |mean| = 1000 std, where the one-sweep rstd is off by 10 %) — so the switch must simply not cost accuracy
    assert max(second) < 1.15 * max(first) and max(second) < 8e-3 and first == unguarded
    # ordinary weights never trip it (the benchmarked configuration keeps its one-sweep statistics)
    encn = DualEncoder(cfg, synth.clip_state_dict(cfg), dtype="bf16", device=DEV)
    for _ in range(3):
        feats(encn)
    assert encn.rowstat_guard_tripped == 0 and encn.vis.rowstats == 2


# ------------------------------------------------------------------------------------------------ device k-means: empty clusters, tolerance
def test_device_kmeans_relocates_an_empty_cluster_and_its_tolerance_is_two_pass():
    """ kmeans_fit on a task with fewer distinct features than clusters used to raise; scikit-learn — and so the reference — relocates the
    empty centre and finishes.  Device fit == the oracle's restatement == scikit-learn.  And the stopping tolerance mean(var(X, 0)) * 1e-4 comes from a
    two-pass column variance: columns whose mean dwarfs their deviation no longer cancel (E[x^2] - mean^2 in f32 went negative there)."""
    import warnings
    from sklearn.cluster import KMeans
    from lpi_amd.kmeans import kmeans_fit
    from oracle import lpi_oracle as O
    x = synth.duplicate_heavy_features()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=5, random_state=0).fit(x)
    centers, labels, iters = kmeans_fit(torch.from_numpy(x).to(DEV), 5, random_state=0)
    c, l = centers.cpu().numpy(), labels.cpu().numpy()
    # every point coincides with a centre here, so "the point farthest from its centre" is a tie among ALL points: which one the relocation takes depends
    # on the last bits of the distances (scikit-learn centres the data first; the device takes exact differences) — the fits agree in what is determined:
    # zero inertia, every distinct feature a centre, labels that point at it
    assert np.isfinite(c).all() and iters <= 20          # a handful of relocations, then the cycle guard (not max_iter = 300)
    assert float(((x - c[l]) ** 2).sum()) < 1e-10 and float(((x - km.cluster_centers_[km.labels_]) ** 2).sum()) < 1e-10
    for row in np.unique(x, axis=0):
        assert np.abs(c - row).sum(1).min() < 1e-6
    oc, ol, oi = O.kmeans_fit(x)                     # the oracle restates scikit-learn's host arithmetic: equal to it on this recipe (CPU test)
    assert float(((x - oc[ol]) ** 2).sum()) < 1e-10
    # tolerance: features riding on a large common offset (|mean| = 1000 x deviation)
    f = synth.clustering_features(600, 64)[0] * 1e-3 + 1.0
    ref = KMeans(n_clusters=5, random_state=0).fit(f)
    c2, l2, it2 = kmeans_fit(torch.from_numpy(f).to(DEV), 5, random_state=0)
    assert it2 == ref.n_iter_ and np.array_equal(l2.cpu().numpy(), ref.labels_)
    assert np.abs(c2.cpu().numpy() - ref.cluster_centers_).max() < 1e-5


# ------------------------------------------------------------------------------------------------ configs[4]'s gather path through bench.py once
def test_bench_vit_l14_four_ranks_on_one_gpu():
    """BASELINE.json configs[4] (ViT-L/14, prompt_depth 12, r 8: E = 768, 12-layer prompt stacks) through bench.py's multi-rank path before the driver's
    8-GPU run meets it: four ranks share this GPU over gloo (host-staged messages), 8 pairs each.  Rank 0's line carries the observed world size, the
    per-rank collective block and the without-exchange self-check; profiles/r05_bench_dp4_vitl14_shared_gpu.json keeps one such line."""
    import subprocess
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "4", "--share-gpu", "--model", "ViT-L/14", "--batch", "8", "--depth", "12",
                        "--rank", "8", "--prompt-layers", "12", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-roofline", "--no-extras"],
                       capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    j = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln][-1])
    c = j["collectives"]
    assert j["n_gpus"] == 4 and c["observed_world_size"] == 4 and c["backend"] == "gloo" and j["config"]["global_batch"] == 32
    assert [r["rank"] for r in c["per_rank"]] == [0, 1, 2, 3] and all(r["median_ms_per_step"] > 0 for r in c["per_rank"])
    assert "1536] f32" in c["messages"] and "14688 factor gradients" in c["messages"]          # E = 768 -> 2E = 1536; 12 x 8 + 2 x 16 x 8 + (1024 + 768) x 8 factors
    assert c["without_exchange"]["value"] > 0 and 0.2 < c["without_exchange"]["ratio_with_exchange"] < 1.5
    assert "ViT-L/14" in j["metric"] and j["value"] > 0
    out = os.path.join(REPO, "gpurun_out")
    if os.path.isdir(out):
        open(os.path.join(out, "bench_dp4_vitl14_shared_gpu.json"), "w").write(json.dumps(j) + "\n")


# ------------------------------------------------------------------------------------------------ persistent GEMM: weight slices (tuning key 15)
@pytest.mark.parametrize("tm,N,K,key", [(43, 3072, 768, 0), (43, 2304, 768, 3), (213, 3072, 768, 0), (20, 3072, 768, 3), (37, 2048, 1024, 2)])
def test_gemm_weight_slices_change_the_order_not_the_bits(tm, N, K, key):
    """Tuning key 15 (round 5): the tiles of a GEMM whose weight does not fit an XCD's L2 run slice-major (2 or 3 slices of the N-tiles, each XCD walking one
    slice after the other down the row panels).  Same tiles, same arithmetic: bit for bit the columns-fastest order (key 15 = -1) — alone, with a bias and
    the derivative epilogue, grouped with a second problem, on shapes with a hybrid half-tile round — and equal to f64 within bf16 rounding."""
    from lpi_amd import engine as E
    from lpi_amd._lib import BF16, call
    M = tm * 256
    g = torch.Generator().manual_seed(tm + N)
    a = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    b = (torch.randn(N, K, generator=g) * 0.05).bfloat16().to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    aux = torch.randn(M, N, generator=g).bfloat16().to(DEV)
    a2 = torch.randn(2560, 512, generator=g).bfloat16().to(DEV)
    b2 = (torch.randn(1536, 512, generator=g) * 0.05).bfloat16().to(DEV)
    s = torch.cuda.current_stream().cuda_stream
    outs = []
    try:
        for k15 in (-1, key):
            call("lpi_set_tuning", 15, k15)
            c0 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            E.gemm(BF16, a, b, c0, M, N, K, bias=bias)
            c1 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            E.gemm(BF16, a, b, c1, M, N, K, epi=E.EPI_DQUICKGELU, aux=aux)
            c2, c3 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV), torch.zeros(2560, 1536, dtype=torch.bfloat16, device=DEV)
            _lib.gemm_grouped(BF16, BF16, E.EPI_NONE, 1.0, [dict(M=M, N=N, K=K, a=a, b=b, c=c2), dict(M=2560, N=1536, K=512, a=a2, b=b2, c=c3)], s)
            torch.cuda.synchronize()
            outs.append((c0, c1, c2, c3))
    finally:
        call("lpi_set_tuning", 15, 0)
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    assert not torch.isnan(outs[1][0].float()).any()
    ref = a.double().cpu() @ b.double().cpu().t() + bias.double().cpu()
    assert float((outs[1][0].double().cpu() - ref).abs().max()) <= 2e-2 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ uint8 pixels
def test_uint8_pixels_give_the_f32_pipelines_features_bit_for_bit():
    """lpi_patchify_u8 (ToTensor + Normalize folded into the im2col through the 3 x 256 table): the im2col columns of uint8 pixels equal lpi_patchify's on
    the host-normalised f32 image bit for bit, in every operand type; so do the image features; and the plugin loop on a u8 dataset (pipeline staging in
    uint8: a quarter of the bytes) trains to the same parameters as on the f32 dataset of the same pixels."""
    from lpi_amd.engine import DualEncoder
    from lpi_amd.retrieval.utils.data import normalise_u8
    from lpi_amd._lib import BF16, F16, F32, call
    g = torch.Generator().manual_seed(5)
    for R, ps, dts in ((32, 16, (F32, BF16, F16)), (224, 16, (BF16,)), (28, 14, (F32,))):
        if ps % 4:
            continue
        B = 3
        u8 = torch.randint(0, 256, (B, 3, R, R), generator=g, dtype=torch.uint8)
        f32 = normalise_u8(u8)
        G, K = R // ps, 3 * ps * ps
        for dt in dts:
            esz = 4 if dt == F32 else 2
            kp = (K + 128 // esz - 1) // (128 // esz) * (128 // esz)
            td = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[dt]
            c0 = torch.zeros(B * G * G, kp, dtype=td, device=DEV)
            c1 = torch.full((B * G * G, kp), 7.0, dtype=td, device=DEV)
            s = torch.cuda.current_stream().cuda_stream
            from lpi_amd.engine import make_pixel_lut
            call("lpi_patchify", dt, B, R, ps, f32.to(DEV), c0, kp, s)
            call("lpi_patchify_u8", dt, B, R, ps, u8.to(DEV), make_pixel_lut().to(DEV), c1, kp, s)
            torch.cuda.synchronize()
            assert torch.equal(c0.view(torch.int32 if esz == 4 else torch.int16), c1.view(torch.int32 if esz == 4 else torch.int16)), (R, ps, dt)
    cfg = synth.TINY
    enc = DualEncoder(cfg, synth.clip_state_dict(cfg), dtype="f32", device=DEV)
    u8 = torch.randint(0, 256, (5, 3, 32, 32), generator=g, dtype=torch.uint8)
    with torch.no_grad():
        fa = enc.encode_image(u8.to(DEV)).clone()
        fb = enc.encode_image(normalise_u8(u8).to(DEV)).clone()
    assert torch.equal(fa, fb)
    # the plugin loop on the two pixel formats of the same pixels
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    ids = torch.from_numpy(synth.token_ids(8, seed=5))
    px = torch.randint(0, 256, (8, 3, 32, 32), generator=g, dtype=torch.uint8)
    got = []
    for fmt in ("u8", "f32"):
        im = px if fmt == "u8" else normalise_u8(px)
        loader = [(im[:4], ids[:4], 0, 0), ([im[j] for j in range(4, 8)], ids[4:], 0, 0)]
        m = SPrompts(tiny_args(epochs=2))
        net = m._network.to(DEV)
        set_factors(net)
        net.numtask = 1
        opt, sch = m._setup_training()
        for ep in range(2):
            m.train_epoch(loader, opt, ep)
            sch.step()
        torch.cuda.synchronize()
        got.append({k: getattr(net.prompts[0], k).detach().clone() for k in synth.PROMPT_NAMES})
        if fmt == "u8":
            assert m._pipeline._stage[0].dtype == torch.uint8 and m._pipeline._dev[0].dtype == torch.uint8
    for k in synth.PROMPT_NAMES:
        assert torch.equal(got[0][k], got[1][k]), k


# ------------------------------------------------------------------------------------------------ the loop's edges
def test_plugin_loop_edges_long_caption_worker_processes_ragged_last_batch(tmp_path, monkeypatch):
    """(a) a caption that does not fit the 77-token context raises RuntimeError like clip.tokenize (clip.py:213-218) — raised in the pipeline's producer
    thread, delivered to the training loop; (b) a DataLoader with WORKER PROCESSES (the reference's num_workers = 8, sprompt.py:166-167: batches arrive stacked in
    shared memory, the pipeline's gather is their pinning copy) and a ragged last batch train to the same parameters as the single-process loader."""
    from torch.utils.data import DataLoader
    from lpi_amd import synth_bpe
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    from lpi_amd.retrieval.models.clip import prompt_learner as PL
    from lpi_amd.retrieval.utils.data import SyntheticCoco, collate_keep_images
    monkeypatch.setenv("LPI_BPE_VOCAB", synth_bpe.write_table(tmp_path / "bpe.txt.gz", seed=2))
    monkeypatch.setattr(PL, "_tokenizer", None)
    m = SPrompts(tiny_args(epochs=1))
    net = m._network.to(DEV)
    set_factors(net)
    net.numtask = 1
    opt, _ = m._setup_training()
    img = torch.from_numpy(synth.images(4, 32))
    bad = [(img, ["a dog", "x " * 80, "a cat", "a bus"], 0, 0)]
    with pytest.raises(RuntimeError, match="too long for context length"):
        m.train_epoch(bad, opt, 0)
    # (b) 10 pairs in batches of 4 (the last one holds 2), caption strings
    ds = SyntheticCoco(10, [0], 32, captions="strings", image_pool=10)
    got = []
    for workers in (0, 2):
        mm = SPrompts(tiny_args(epochs=2))
        nn_ = mm._network.to(DEV)
        set_factors(nn_)
        nn_.numtask = 1
        o, sch = mm._setup_training()
        loader = DataLoader(ds, batch_size=4, shuffle=False, num_workers=workers, collate_fn=collate_keep_images if workers == 0 else None)
        seen = []
        for ep in range(2):
            mm.train_epoch(loader, o, ep, None, lambda i, b, out: seen.append(b.images.shape[0]) and False)
            sch.step()
        torch.cuda.synchronize()
        assert seen == [4, 4, 2, 4, 4, 2]
        got.append({k: getattr(nn_.prompts[0], k).detach().clone() for k in synth.PROMPT_NAMES})
        del loader
    for k in synth.PROMPT_NAMES:
        assert torch.equal(got[0][k], got[1][k]), k
    monkeypatch.setattr(PL, "_tokenizer", None)


# ------------------------------------------------------------------------------------------------ the f16 mode against the reference in its own fp16
@pytest.mark.parametrize("fx,f32fx,cfgname,batch", [("tiny_fp16", "tiny_d1", "tiny", 4), ("vitb16_fp16", "vitb16_d1", "ViT-B/16", 8)])
def test_f16_mode_against_the_reference_run_in_its_own_fp16(golden, fx, f32fx, cfgname, batch):
    """compute_dtype='f16' is "the reference's own arithmetic type" (model.py:394-415): here it is held against the reference actually RUN in that type
    (tests/golden/*_fp16.npz: convert_weights applied, torch CPU fp16 kernels).  Two fp16 evaluations of the same network differ by their accumulation
    orders, so the bar is fp16 rounding — and the HIP f16 step must be at least as close to the f32 reference as the reference's own fp16 run is (f32
    accumulation, f32 LayerNorm statistics and softmax here)."""
    from lpi_amd.engine import DualEncoder
    from lpi_amd.step import train_step
    cfg = synth.CONFIGS[cfgname]
    g16, g32 = golden(fx), golden(f32fx)
    enc = DualEncoder(cfg, synth.clip_state_dict(cfg), dtype="f16", device=DEV)
    fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
    img = torch.from_numpy(synth.images(batch, cfg.image_resolution)).to(DEV)
    out = train_step(enc, img, torch.from_numpy(g16["token_ids"]).to(DEV), fac, 1)
    torch.cuda.synchronize()
    mx = lambda a, b: float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())  # noqa: E731
    hip = {"img_f": out["img_f"].cpu().numpy(), "txt_f": out["txt_f"].cpu().numpy(),
           "logits": (enc.logit_scale_exp * out["img_f"] @ out["txt_f"].t()).cpu().numpy()}
    d = {k: (mx(hip[k], g16[k]), mx(hip[k], g32[k]), mx(g16[k], g32[k])) for k in hip}
    print(f"\n    {cfgname}: max |HIP f16 - ref fp16|, |HIP f16 - ref f32|, |ref fp16 - ref f32|: " + ", ".join(f"{k} {a:.2e} {b:.2e} {c:.2e}" for k, (a, b, c) in d.items()))
    for k, bar in (("img_f", 1e-3), ("txt_f", 1e-3), ("logits", 1e-2)):
        assert d[k][0] < bar, (k, d[k])
        assert d[k][1] < 2.0 * d[k][2] + 1e-4, (k, d[k])          # as close to the f32 reference as the reference's own fp16 run (within 2x)
    assert abs(float(out["base_loss"]) - float(g16["base_loss"])) < 3e-3 * max(1.0, abs(float(g16["base_loss"])))
    for k in synth.PROMPT_NAMES:
        a, r16, r32 = fac[k].grad.cpu().numpy().astype(np.float64), g16["grad." + k].astype(np.float64), g32["grad." + k].astype(np.float64)
        cos = lambda x, y: float((x * y).sum() / np.sqrt((x * x).sum() * (y * y).sum()))  # noqa: E731
        assert cos(a, r16) > 0.998 and cos(a, r32) > 0.998, (k, cos(a, r16), cos(a, r32))


def test_fused_plugin_step_at_vitb16_size_matches_the_reference_fixture(golden):
    """BASELINE.json configs[0]'s shape through the PLUGIN's fused step: SliNet(configs/lpi/coco_lpi.json, ViT-B/16, f32).train_step on 8 pairs against the
    imported reference's outputs (tests/golden/vitb16_d1.npz: the shipped code, effective prompt depth 1) — features and logits to 1e-4, losses to 1e-4,
    factor gradients to 1e-3 relative — and the top-5 retrieval indices wherever the reference's recorded margin exceeds 10x the measured logit error."""
    from lpi_amd.retrieval.models.slinet import SliNet
    g = golden("vitb16_d1")
    args = json.load(open(os.path.join(RET, "configs", "lpi", "coco_lpi.json")))
    args.update(device=[DEV], compute_dtype="f32")
    net = SliNet(args).to(DEV)
    cfg = net.clip_cfg
    for t in range(len(net.prompts)):
        for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width, task=t).items():
            getattr(net.prompts[t], k).data = torch.from_numpy(v.copy()).to(DEV)
    net.numtask = 1
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad_("prompts.0." in n)
    img = torch.from_numpy(synth.images(8, cfg.image_resolution)).to(DEV)
    out = net.train_step(img, torch.from_numpy(g["token_ids"]))
    torch.cuda.synchronize()
    fi, ft = out["image_features"], out["text_features"]
    assert float((fi.cpu() - torch.from_numpy(g["img_f"])).abs().max()) < 1e-4 and float((ft.cpu() - torch.from_numpy(g["txt_f"])).abs().max()) < 1e-4
    logits = (net.engine.logit_scale_exp * fi @ ft.t()).cpu().numpy()
    err = float(np.abs(logits - g["logits"]).max())
    assert err < 1e-4
    for k in ("base_loss", "alignment_loss"):
        assert abs(float(out["loss"][k]) - float(g[k])) < 1e-4
    for k in synth.PROMPT_NAMES:
        got, ref = getattr(net.prompts[0], k).grad.cpu().numpy(), g["grad." + k]
        assert np.abs(got - ref).max() <= 1e-3 * np.abs(ref).max() + 1e-7, k
    for tag, S in (("i2t", logits), ("t2i", logits.T)):
        idx = np.argsort(-S, axis=1, kind="stable")[:, : g[f"top5_{tag}"].shape[1]]
        safe = g[f"top5_margin_{tag}"] > 10 * err
        assert safe.mean() > 0.5 and (idx[safe] == g[f"top5_{tag}"][safe]).all()
