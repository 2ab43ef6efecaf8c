"""CPU: the segmentation's host side -- gen_patches' cuts, the float64 restatement of the network against the reference's
own torch run (tests/golden/ref_segment.npz), the torch-free weights reader against torch.load (torch in a subprocess
only: never in the pytest process), the parameter folding and the argument refusals."""
import os
import subprocess
import sys
import textwrap
from collections import OrderedDict

import numpy as np
import pytest

import _unet_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ref_segment.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def test_param_spec_is_the_references_state_dict(gold):
    from invesalius3_amd.segment import param_spec
    spec = param_spec()
    assert [k for k, _ in spec] == list(gold["param_names"])
    shapes, cur = [], []
    for v in gold["param_shapes"]:
        if v == -1:
            shapes.append(tuple(cur))
            cur = []
        else:
            cur.append(int(v))
    assert [s for _, s in spec] == shapes
    assert "decoder1.dec4_conv1.weight" in dict(spec)  # model.py:49 reuses the dec4_ prefix


def test_weights_regenerate_from_the_seed(gold):
    assert R.weights_crc(R.make_weights()) == int(gold["weights_crc"]), "the numpy random stream changed"


def test_cuts_equal_gen_patches(gold):
    from invesalius3_amd.segment import gen_patches, patch_cuts
    for i, case in enumerate(gold["cut_cases"]):
        shp, ov, P = str(case).split("|")
        shp = tuple(int(s) for s in shp.split(","))
        want = [((a, b), (c, d), (e, f)) for a, b, c, d, e, f in gold["cuts_%d" % i].tolist()]
        assert patch_cuts(shp, int(P), int(ov)) == want, case
    img = np.arange(5 * 6 * 7, dtype=np.float32).reshape(5, 6, 7)
    got = [(c, p.copy()) for _, p, c in gen_patches(img, 16, 50)]
    assert len(got) == 1 and got[0][0] == ((0, 5), (0, 6), (0, 7))
    assert np.array_equal(got[0][1][:5, :6, :7], img) and not got[0][1][5:].any()


def test_float64_restatement_against_the_reference(gold):
    """the reference's float32 torch run agrees with the float64 restatement within the bound, and so does the mask
    rule: the masks differ only where the reference's p lies within the bound of float32(0.75)"""
    sd = R.make_weights()
    thr = np.float32(0.75)
    for case in gold["seg_cases"]:
        name, P, ov, wwwl, ww, wl = str(case).split("|")
        P, ov = int(P), int(ov)
        vol, pref, mref = gold["vol_" + name], gold["prob_" + name], gold["mask_" + name]
        img = R.get_lut_value(vol, int(ww), int(wl)) if int(wwwl) else vol
        from invesalius3_amd.segment import gen_patches, image_normalize_f32
        nrm = image_normalize_f32(img)
        outs = [R.forward64(sd, p) for _, p, _ in gen_patches(nrm, P, ov)]
        p64 = R.accumulate(nrm, P, ov, [o.astype(np.float32) for o in outs])
        assert float(np.abs(p64.astype(np.float64) - pref).max()) <= 5e-5, name
        m = np.zeros_like(mref)
        m[1:, 1:, 1:] = (p64 >= thr) * 255
        m[:, 0, 0] = m[0, :, 0] = m[0, 0, :] = 2
        diff = m != mref
        assert not diff[0].any() and not diff[:, 0].any() and not diff[:, :, 0].any()
        assert (np.abs(pref[diff[1:, 1:, 1:]] - thr) <= 5e-5).all(), name
        if name == "a":
            frac = (pref >= thr).mean()
            assert 0.05 <= frac <= 0.95  # the weights straddle the GUI default


def test_normalisation_is_numpys_with_both_wraps():
    from invesalius3_amd.segment import image_normalize_f32
    a = np.array([-20000, 0, 20000], np.int16)
    got = image_normalize_f32(a)
    with np.errstate(over="ignore"):
        d = np.int16(20000) - np.int16(-20000)
        assert d < 0  # imax - imin wraps
        want = ((a - np.int16(-20000)) * (1.0 / d) + 0.0).astype(np.float32)
    assert np.array_equal(got, want)
    assert not image_normalize_f32(np.full((2, 2), 5, np.int16)).any()


def _torch(code, tmp_path):
    """run `code` in a torch subprocess (torch bundles its own HIP runtime: never in this process)"""
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_pt_reader_against_torch_load(tmp_path):
    from invesalius3_amd.segment import load_weights
    _torch("""
        import collections, torch
        base = torch.arange(60, dtype=torch.float32).reshape(6, 10)
        sd = collections.OrderedDict()
        sd["w"] = torch.randn(3, 4, 5, generator=torch.Generator().manual_seed(1))
        sd["view"] = base[1:5, 2:9:3]                  # a strided view with a storage offset
        sd["shared"] = base[2]                         # the same storage again
        sd["i64"] = torch.tensor(1234567890123, dtype=torch.int64)
        sd["i32"] = torch.arange(7, dtype=torch.int32)
        sd["f64"] = torch.linspace(0, 1, 5, dtype=torch.float64)
        sd["p"] = torch.nn.Parameter(torch.ones(2, 2))
        torch.save({"model_state_dict": sd, "epoch": 3}, "nested.pt")
        torch.save(sd, "plain.pt")
        import numpy as np
        np.savez("ref.npz", **{k: v.detach().numpy() for k, v in sd.items()})
    """, tmp_path)
    with np.load(tmp_path / "ref.npz") as z:
        ref = {k: z[k] for k in z.files}
    for f in ("nested.pt", "plain.pt"):
        got = load_weights(tmp_path / f)
        assert list(got) == list(ref)
        for k in ref:
            assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (f, k)
    assert load_weights(tmp_path / "ref.npz").keys() == ref.keys()
    assert load_weights({"model_state_dict": OrderedDict(a=np.ones(2))})["a"].tolist() == [1.0, 1.0]


def test_pt_reader_refusals(tmp_path):
    from invesalius3_amd.segment import load_weights
    _torch("""
        import os, pickle, torch, zipfile
        torch.save({"x": torch.ones(2)}, "legacy.pt", _use_new_zipfile_serialization=False)
        # a torch.save archive whose pickle names a global outside the whitelist
        class Evil:
            def __reduce__(self):
                return (os.system, ("echo pwned > pwned.txt",))
        torch.save({"x": torch.ones(2)}, "evil.pt")
        with zipfile.ZipFile("evil.pt") as z:
            items = [(n, z.read(n)) for n in z.namelist()]
        with zipfile.ZipFile("evil.pt", "w") as z:
            for n, b in items:
                z.writestr(n, pickle.dumps({"x": Evil()}, protocol=2) if n.endswith("data.pkl") else b)
    """, tmp_path)
    import pickle
    with pytest.raises(ValueError, match="legacy"):
        load_weights(tmp_path / "legacy.pt")
    with pytest.raises(pickle.UnpicklingError, match="forbidden global"):
        load_weights(tmp_path / "evil.pt")
    assert not (tmp_path / "pwned.txt").exists()
    with pytest.raises(FileNotFoundError):
        load_weights(tmp_path / "missing.pt")
    (tmp_path / "junk.pt").write_bytes(b"not a weights file")
    with pytest.raises(ValueError):
        load_weights(tmp_path / "junk.pt")


def test_strict_keys_and_folding():
    from invesalius3_amd import segment as sg
    sd = R.make_weights()
    chk = sg.check_state_dict(sd)
    assert list(chk) == [k for k, _ in sg.param_spec()]
    missing = dict(sd)
    del missing["decoder2.dec4_norm1.running_var"]
    with pytest.raises(RuntimeError, match="Missing key"):
        sg.check_state_dict(missing)
    extra = dict(sd, **{"decoder2.dec2_conv1.weight": np.zeros(1)})  # the "tidied" name the real files do not use
    with pytest.raises(RuntimeError, match="Unexpected key"):
        sg.check_state_dict(extra)
    bad = dict(sd, **{"conv.bias": np.zeros(2, np.float32)})
    with pytest.raises(RuntimeError, match="size mismatch"):
        sg.check_state_dict(bad)


def test_fold_params_layout(ivx_lib_loaded):
    """the blob: BatchNorm folded in float64 and rounded once, in the header's order"""
    from invesalius3_amd import segment as sg
    sd = R.make_weights()
    blob = sg.fold_params(sd)
    g = lambda k: sd[k].astype(np.float64)  # noqa: E731
    s = g("encoder1.enc1_norm1.weight") / np.sqrt(g("encoder1.enc1_norm1.running_var") + 1e-5)
    w = (g("encoder1.enc1_conv1.weight") * s[:, None, None, None, None]).astype(np.float32).ravel()
    b = ((g("encoder1.enc1_conv1.bias") - g("encoder1.enc1_norm1.running_mean")) * s + g("encoder1.enc1_norm1.bias")).astype(np.float32)
    assert np.array_equal(blob[:w.size], w) and np.array_equal(blob[w.size:w.size + 8], b)
    assert np.array_equal(blob[-9:-1], sd["conv.weight"].ravel()) and blob[-1] == sd["conv.bias"][0]


@pytest.fixture
def ivx_lib_loaded():
    from invesalius3_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("patch,overlap", [(24, 50), (0, 50), (8, 0), (48, 100), (48, -1), (48, 150)])
def test_argument_refusals(patch, overlap):
    from invesalius3_amd import segment as sg
    with pytest.raises(ValueError):
        sg.patch_cuts((48, 48, 48), patch, overlap)
    with pytest.raises(ValueError):
        list(sg.gen_patches(np.zeros((8, 8, 8), np.float32), patch, overlap))


def test_presets():
    from invesalius3_amd.segment import PRESETS
    assert PRESETS["brain"].weights_file_name == "brain_mri_t1.pt"
    assert PRESETS["trachea"].weights_file_name == "trachea_ct.pt"
    for p in PRESETS.values():
        assert (p.patch_size, p.overlap, p.threshold, p.mask_name_pattern) == (48, 50, 0.75, "brainseg_mri_t1")
