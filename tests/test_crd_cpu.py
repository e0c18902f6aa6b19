"""CPU checks of the `--distill crd` path: the numpy restatement of the CRD formulas (tests/crd_ref.py) against the golden fixture
recorded from the reference, the synthetic sample loader, the alias tables, the construction of the training objects, and the
refusal of CPU tensors by the kernel wrappers.  (The C ABI's table-driven argument test in tests/test_abi_cpu.py picks the new entry
points up by itself.)"""
import os

import numpy as np
import pytest
import torch

from tests import crd_ref as R, golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g11():
    return golden_npz.load(os.path.join(ROOT, "tests", "golden", "g11_crd.npz"))


def test_fixture_files_stay_below_the_size_limit():
    import glob
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "g11_crd*.npz"))
    assert files and all(os.path.getsize(f) < (1 << 20) for f in files)


def test_restatement_reproduces_the_reference(g11):
    """float64 evaluation of the formulas vs the reference's fp32 results: within the distances the generator recorded, and those
    are fp32 rounding noise (so the formulas ARE the reference's computation)"""
    assert int(g11["n_cases"]) == 3
    for ci in range(3):
        p = f"c{ci}_"
        B, d, K, n_data, s_dim, t_dim, steps, rep = (int(v) for v in g11[p + "shape"])
        m1, m2 = g11[p + "memory_v1"].astype(np.float64), g11[p + "memory_v2"].astype(np.float64)
        assert g11[p + "ref_vs_f64_loss"] < 5e-5 and g11[p + "ref_vs_f64_dv"] < 1e-5 and g11[p + "ref_vs_f64_z"] < 1e-6
        for st in range(steps):
            q = f"{p}s{st}_"
            idx, params = g11[q + "idx"].astype(np.int64), g11[q + "params"]
            y = idx[:, 0]
            assert params[0] == K and params[2] > 0 and params[3] > 0
            if st > 0:
                assert np.array_equal(params, g11[f"{p}s0_params"])          # Z is set by the first step only
            if rep:
                assert len(set(y.tolist())) < B
            T, mom = float(params[1]), float(params[4])
            v1, c1 = R.embed(g11[q + "f_s"], g11[p + "ws"], g11[p + "bs"])
            v2, c2 = R.embed(g11[q + "f_t"], g11[p + "wt"], g11[p + "bt"])
            s1, s2 = R.side(v1, m2, idx, T, float(params[2])), R.side(v2, m1, idx, T, float(params[3]))
            assert R.rel(g11[q + "out_v1"], s1["x"]) <= g11[p + "ref_vs_f64_out"]
            assert R.rel(g11[q + "out_v2"], s2["x"]) <= g11[p + "ref_vs_f64_out"]
            assert abs(g11[q + "loss"][0] - s1["loss"]) <= g11[p + "ref_vs_f64_loss"] * abs(s1["loss"])
            assert abs(g11[q + "loss"][1] - s2["loss"]) <= g11[p + "ref_vs_f64_loss"] * abs(s2["loss"])
            assert R.rel(g11[q + "dv1"], s1["dv"]) <= g11[p + "ref_vs_f64_dv"]
            assert R.rel(g11[q + "dv2"], s2["dv"]) <= g11[p + "ref_vs_f64_dv"]
            dws, dbs = R.embed_bwd(s1["dv"], c1)
            assert R.rel(g11[q + "dws"], dws) <= g11[p + "ref_vs_f64_dw"] and R.rel(g11[q + "dbs"], dbs) <= g11[p + "ref_vs_f64_db"]
            # the materialised backward restated: dout of ContrastLoss through scores_bwd equals the fused gradient
            c = K / n_data
            g = np.empty_like(s1["x"])
            g[:, 0] = -(1 / s1["x"][:, 0] - 1 / (s1["x"][:, 0] + c + R.EPS)) / B
            g[:, 1:] = 1 / (s1["x"][:, 1:] + c + R.EPS) / B
            assert R.rel(R.scores_bwd(g, s1["x"], m2, idx, T), s1["dv"]) < 1e-12
            if st == 0:
                z1 = R.z_of(s1["e"], n_data)
                assert abs(float(params[2]) - z1) / z1 <= g11[p + "ref_vs_f64_z"]
            n1, n2 = R.update(m1, v1, y, mom), R.update(m2, v2, y, mom)
            assert R.rel(g11[q + "rows_v1"], n1[y]) <= g11[p + "ref_vs_f64_rows"]
            assert R.rel(g11[q + "rows_v2"], n2[y]) <= g11[p + "ref_vs_f64_rows"]
            m1, m2 = n1, n2
            m1[y], m2[y] = g11[q + "rows_v1"], g11[q + "rows_v2"]          # continue from the reference's fp32 banks


def test_restatement_skips_indices_that_are_no_rows():
    rng = np.random.default_rng(0)
    M, v = rng.standard_normal((50, 8)), rng.standard_normal((3, 8))
    idx = rng.integers(0, 50, (3, 9))
    a = R.side(v, M, idx, 0.5, 40.0)
    idx2 = np.concatenate([idx, np.full((3, 1), 50)], 1)
    idx2[1, -1] = -1
    e2, ok, _ = R.scores(v, M, idx2, 0.5)
    assert not ok[:, -1].any() and (e2[:, -1] == 0).all()
    assert np.allclose(R.scores(v, M, idx2, 0.5)[0][:, :-1], a["e"])


@pytest.mark.parametrize("mode", ["exact", "relax"])
def test_sample_loader(mode):
    from moma_amd.dataset.synthetic import SyntheticSampleLoader
    mk = lambda seed: SyntheticSampleLoader(5, 16, 8, 4, 64, mode, seed, "cpu")       # noqa: E731
    ld = mk(3)
    assert len(ld) == 5 and ld.n_data == 80
    seen, batches = [], list(ld)
    for images, labels, index, cidx in batches:
        assert images.shape == (16, 3, 8, 8) and labels.shape == (16,) and labels.dtype == torch.int64
        assert index.dtype == torch.int64 and cidx.dtype == torch.int64 and cidx.shape == (16, 65)
        assert torch.equal(cidx[:, 0], index) and len(set(index.tolist())) == 16
        assert int(cidx.min()) >= 0 and int(cidx.max()) < 80
        assert torch.equal(labels, ld.sample_labels[index])
        neg = cidx[:, 1:]
        if mode == "exact":
            assert not (ld.sample_labels[neg] == labels[:, None]).any()           # negatives come from the OTHER classes
        else:
            assert not (neg == index[:, None]).any()                               # ... or from all OTHER samples
        seen += index.tolist()
    assert sorted(seen) == list(range(80))                                         # the epoch walks a permutation of the set
    again = list(mk(3))
    assert all(torch.equal(a[3], b[3]) and torch.equal(a[2], b[2]) for a, b in zip(batches, again))     # seeded
    other = list(mk(4))
    assert any(not torch.equal(a[3], b[3]) for a, b in zip(batches, other))
    # every admissible negative can be drawn: over many draws the union covers the whole complement
    big = SyntheticSampleLoader(1, 4, 8, 3, 4000, mode, 1, "cpu", n_data=40)
    _, labels, index, cidx = next(iter(big))
    for b in range(4):
        want = {i for i in range(40) if (big.sample_labels[i] != labels[b] if mode == "exact" else i != int(index[b]))}
        assert set(cidx[b, 1:].tolist()) == want
    with pytest.raises(ValueError):
        SyntheticSampleLoader(1, 16, 8, 4, 8, "nearest", 0, "cpu")
    with pytest.raises(ValueError):
        SyntheticSampleLoader(1, 16, 8, 4, 8, mode, 0, "cpu", n_data=8)


def test_alias_tables_sum_to_the_distribution():
    from moma_amd.crd import AliasMethod
    for probs in (np.ones(37), np.array([0.5, 0.1, 0.1, 0.3]), np.random.default_rng(2).random(101)):
        a = AliasMethod(torch.from_numpy(probs.astype(np.float32)))
        n = len(probs)
        p = probs / probs.sum() if probs.sum() > 1 else probs
        prob, alias = a.prob.double().numpy(), a.alias.numpy()
        assert ((prob >= 0) & (prob <= 1 + 1e-6)).all() and ((alias >= 0) & (alias < n)).all()
        back = prob / n
        np.add.at(back, alias, (1 - prob) / n)
        assert np.allclose(back, p, atol=1e-6) and abs(back.sum() - p.sum()) < 1e-6
    torch.manual_seed(0)
    d = AliasMethod(torch.tensor([0.5, 0.1, 0.1, 0.3])).draw(40000)
    assert d.dtype == torch.int64 and np.allclose(np.bincount(d.numpy(), minlength=4) / 40000, [0.5, 0.1, 0.1, 0.3], atol=0.01)


def test_build_training_with_distill_crd():
    from moma_amd.train_student_moma import build_training, parse_option
    from moma_amd.crd import CRDLoss
    opt = parse_option(["--distill", "crd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
                        "--n_cls", "4", "--batch_size", "8", "--steps_per_epoch", "5", "--nce_k", "32", "--feat_dim", "64", "-b", "0.8"])
    opt.gpu, opt.multiprocessing_distributed = 0, False
    torch.manual_seed(0)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = build_training(opt, torch.device("cpu"))
    kd = criterion_list[2]
    assert isinstance(kd, CRDLoss) and contrast is None and opt.n_data == 40 and opt.nce_t == 0.07
    assert any(m is kd.embed_s for m in trainable_list) and any(m is kd.embed_t for m in trainable_list)      # both heads train
    assert any(m is kd.embed_s for m in module_list) and any(m is kd.embed_t for m in module_list) and module_list[-1] is model_t
    opt_params = {id(p) for g in optimizer.param_groups for p in g["params"]}
    assert all(id(p) in opt_params for p in kd.embed_t.parameters()) and all(p.requires_grad for p in kd.embed_t.parameters())
    assert not any(id(p) in opt_params for p in model_t.parameters())
    keys = set(kd.state_dict())
    assert {"contrast.memory_v1", "contrast.memory_v2", "contrast.params", "embed_s.linear.weight", "embed_s.linear.bias",
            "embed_t.linear.weight", "embed_t.linear.bias"} == keys
    assert kd.contrast.memory_v1.shape == (40, 64) and kd.embed_s.linear.in_features == opt.s_dim
    assert kd.contrast.params.tolist()[0] == 32 and kd.contrast.params.tolist()[2:4] == [-1, -1]
    stdv = 1 / np.sqrt(64 / 3)
    assert float(kd.contrast.memory_v1.abs().max()) <= stdv and float(kd.contrast.memory_v1.abs().max()) > 0.9 * stdv
    opt2 = parse_option(["--distill", "crd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
                         "--n_cls", "4", "--batch_size", "8", "--nce_k", "32", "--feat_dim", "64", "--n_data", "123"])
    opt2.gpu, opt2.multiprocessing_distributed = 0, False
    assert build_training(opt2, torch.device("cpu"))[3][2].contrast.memory_v2.shape == (123, 64)
    # a state dict round trip makes the module look at `params` again (Z already set -> not set a second time)
    sd = kd.state_dict()
    sd["contrast.params"] = torch.tensor([32, 0.07, 5.0, 6.0, 0.5])
    kd.load_state_dict(sd)
    assert kd.contrast._state() == [32, pytest.approx(0.07), 0.5, False]


def test_crd_ops_refuse_cpu_tensors():
    from moma_amd import _lib, ops
    from moma_amd.crd import ContrastMemory
    from moma_amd import build
    build.build(verbose=False)
    v, M = torch.zeros(2, 8), torch.zeros(10, 8)
    idx, Z, bad = torch.zeros(2, 5, dtype=torch.int64), torch.ones(2), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.MomaHipError):
        ops.crd_fused(v, v, M, M, idx, 0.07, 10, Z, True, bad)
    with pytest.raises(_lib.MomaHipError):
        ops.crd_scores(v, v, M, M, idx, 0.07, 10, Z, True, bad)
    with pytest.raises(_lib.MomaHipError):
        ops.crd_update_(M, M.clone(), v, v, idx[:, 0].contiguous(), 0.5, bad)
    mem = ContrastMemory(8, 10, 4)
    with pytest.raises(_lib.MomaHipError):
        mem.forward_fused(v, v, idx[:, 0].contiguous())
    with pytest.raises(_lib.MomaHipError):
        mem(v, v, idx[:, 0].contiguous(), idx)


def test_crd_workspace_query():
    import ctypes
    from moma_amd import _lib
    lib = _lib.load()
    f = lib.moma_crd_workspace_bytes
    assert f(64, 512, 16385) >= 2 * 64 * 512 * 4 and f(1, 64, 2) > 0
    assert f(64, 510, 16385) == 0 and f(64, 4096, 16385) == 0 and f(64, 512, 1) == 0 and f(0, 512, 100) == 0
    assert f(64, 512, 16385) == f(64, 512, 16385)
