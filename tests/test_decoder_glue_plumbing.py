"""CPU tier: the plumbing of the decoder glue with bias + ELU inside (ops.upcat_pad_act, ops.bias_elu_pad,
ops.FUSED_DECODER_GLUE).  The kernels themselves: tests/test_gpu_decoder_glue.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

NEW_SYMBOLS = ("bbd_upcat_pad_act_fwd", "bbd_upcat_pad_act_bwd", "bbd_bias_elu_pad_fwd", "bbd_bias_elu_pad_bwd")


def _decoder_run(dec, feats, glue, monkeypatch):
    from baseboostdepth_amd import ops
    reached = []
    with monkeypatch.context() as m:
        m.setattr(ops, "FUSED_DECODER_GLUE", glue)
        for name in ("upcat_pad_act", "bias_elu_pad", "upcat_pad", "bias_elu_", "reflect_pad1"):
            m.setattr(ops, name, lambda *a, _n=name, **k: reached.append(_n))
        xs = [t.clone().requires_grad_(True) for t in feats]
        for p in dec.parameters():
            p.grad = None
        out = dec(xs)
        disps = [out[("disp", s)] for s in range(4)]
        sum((d * (s + 1.0)).sum() for s, d in enumerate(disps)).backward()
    assert reached == []                                        # host tensors: the eager path, whatever the switch says
    return [d.detach() for d in disps] + [t.grad for t in xs] + [p.grad.clone() for p in dec.parameters()]


def test_depth_decoder_on_host_tensors_is_the_same_with_the_switch_on_and_off(monkeypatch):
    from baseboostdepth_amd import networks
    torch.manual_seed(0)
    enc = [4, 4, 8, 8, 16]
    dec = networks.DepthDecoder(enc, [0, 1, 2, 3]).train()
    feats = [torch.randn(2, c, 64 >> (i + 1), 64 >> (i + 1)) for i, c in enumerate(enc)]
    on = _decoder_run(dec, feats, True, monkeypatch)
    off = _decoder_run(dec, feats, False, monkeypatch)
    assert len(on) == len(off) == 4 + 5 + 28
    for a, b in zip(on, off):
        assert torch.equal(a, b)


def test_the_switch_is_read_from_the_environment():
    code = "from baseboostdepth_amd import ops; print(int(ops.FUSED_DECODER_GLUE))"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in ((None, "1"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "BBD_FUSED_DECODER_GLUE"}
        if value is not None:
            env["BBD_FUSED_DECODER_GLUE"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want


def test_library_exports_the_new_entry_points():
    from baseboostdepth_amd import _lib
    from baseboostdepth_amd.csrc.build import build
    dll = ctypes.CDLL(build())
    for name in NEW_SYMBOLS:
        assert hasattr(dll, name) and _lib.PROTOTYPES[name].has_stream and _lib.PROTOTYPES[name].restype is ctypes.c_int
    assert _lib.GLUE_ROWS == 4 and _lib.ABI_VERSION >= 22
    assert [n for _, n in _lib.PROTOTYPES["bbd_upcat_pad_act_bwd"].params][6:8] == ["scratch", "scratch_doubles"]
    assert [n for _, n in _lib.PROTOTYPES["bbd_bias_elu_pad_bwd"].params][5:7] == ["scratch", "scratch_doubles"]


def test_the_new_ops_refuse_host_tensors():
    from baseboostdepth_amd import ops, _lib
    z, bias = torch.randn(1, 2, 2, 4), torch.randn(2)
    assert not ops.upcat_pad_act_supported(z, bias, None) and not ops.bias_elu_pad_supported(z, bias)
    with pytest.raises(_lib.BbdError):
        ops.upcat_pad_act(z, bias, torch.randn(1, 1, 4, 8))
    with pytest.raises(_lib.BbdError):
        ops.bias_elu_pad(z * 1.0, bias)
