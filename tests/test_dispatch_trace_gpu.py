"""Which extension kernels one training step launches, and with what.

Every callable of the HIP extension is wrapped; each call is recorded as
``[phase, name, args]`` where a tensor argument (lists flattened) becomes
``["T", shape, dtype]`` and an int/bool/float argument its value.  One
forward + ``DistributedRelativeLpLoss`` + backward of ``DistributedFNONd`` on
a single-rank partition is compared with ``tests/golden/dispatch_trace.json``:
forward calls in order, backward calls as a sorted multiset (independent
autograd nodes may legitimately swap).

The golden file pins the host-side dispatch: it was recorded once, from the
commit named in its ``recorded_from`` entry, by running this module as a
script with ``--record`` on a GPU.  It is not regenerated when the Python
dispatch is restructured -- that is the change it guards against.
"""

import json
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "dispatch_trace.json"

IN_SHAPE = [1, 2, 8, 8, 8, 1]
OUT_T = 10
MODES = (2, 2, 2, 3)

# name -> (dtype, width, env, backward)
CASES = {
    "fp32_w20": ("float32", 20, {}, True),
    "fp32_w8": ("float32", 8, {}, True),
    "fp32_w20_rfft_adj_off": ("float32", 20, {"DFNO_FUSED_RFFT_ADJ": "0"}, True),
    "fp32_w20_epilogue_off": ("float32", 20, {"DFNO_FUSED_EPILOGUE": "0"}, True),
    "fp32_w8_zt": ("float32", 8, {"DFNO_ZT": "1"}, True),
    "bf16_w20": ("bfloat16", 20, {}, True),
    "bf16_w8": ("bfloat16", 8, {}, True),
    "fp64_w8": ("float64", 8, {}, True),
    "fp32_w20_no_grad": ("float32", 20, {}, False),
}
KNOBS = ("DFNO_ZT", "DFNO_FUSED_EPILOGUE", "DFNO_FUSED_RFFT_ADJ",
         "DFNO_PIPELINE_CHUNKS")


def _describe(args, out):
    for a in args:
        if isinstance(a, torch.Tensor):
            out.append(["T", list(a.shape), str(a.dtype).replace("torch.", "")])
        elif isinstance(a, (list, tuple)):
            _describe(a, out)
        elif isinstance(a, (bool, int, float)):
            out.append(a)
        else:
            out.append(None if a is None else repr(a))
    return out


def _trace(case, monkeypatch):
    import dfno_amd as dfno
    from dfno_amd import _ext, dispatch
    from dfno_amd.ops.fft import _GRAD_STASH

    dtype_name, width, env, backward = CASES[case]
    dtype = getattr(torch, dtype_name)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)

    ext = _ext.get(required=True)
    calls = []
    phase = ["fwd"]

    def wrap(name, fn):
        def wrapped(*args, **kwargs):
            desc = _describe(args, [])
            for k in sorted(kwargs):
                _describe([kwargs[k]], desc)
            calls.append([phase[0], name, desc])
            return fn(*args, **kwargs)
        return wrapped

    for name in dir(ext):
        fn = getattr(ext, name)
        if not name.startswith("__") and callable(fn):
            monkeypatch.setattr(ext, name, wrap(name, fn))

    dispatch.reset_fallbacks()
    device = torch.device("cuda:0")
    torch.manual_seed(3)
    _, P_x, _ = dfno.create_standard_partitions((1, 1, 1, 1, 1, 1))
    model = dfno.DistributedFNONd(P_x, IN_SHAPE, OUT_T, width, MODES,
                                  num_blocks=2, device=device, dtype=dtype)
    torch.manual_seed(4)
    x = torch.rand(*IN_SHAPE, device=device, dtype=dtype)
    if backward:
        y = model(x)
        tgt = torch.rand_like(y)
        loss = dfno.DistributedRelativeLpLoss(P_x)(y, tgt)
        phase[0] = "bwd"
        loss.backward()
    else:
        with torch.no_grad():
            y = model(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    dispatch.assert_all_native()
    assert not _GRAD_STASH, "stash entry left behind"
    return calls


def _split(calls):
    fwd = [c for c in calls if c[0] == "fwd"]
    bwd = sorted((c for c in calls if c[0] == "bwd"),
                 key=lambda c: json.dumps(c))
    return fwd, bwd


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())["cases"]


@pytest.mark.parametrize("case", list(CASES))
def test_dispatch_trace(case, golden, monkeypatch):
    calls = json.loads(json.dumps(_trace(case, monkeypatch)))
    assert calls, "no extension call recorded"
    fwd, bwd = _split(calls)
    ref_fwd, ref_bwd = _split(golden[case])
    assert len(fwd) == len(ref_fwd), \
        f"forward: {[c[1] for c in fwd]} vs {[c[1] for c in ref_fwd]}"
    for i, (a, b) in enumerate(zip(fwd, ref_fwd)):
        assert a == b, f"forward call {i}: {a} vs golden {b}"
    assert [c[1] for c in bwd] == [c[1] for c in ref_bwd], \
        "backward: different set of kernels"
    for a, b in zip(bwd, ref_bwd):
        assert a == b, f"backward call: {a} vs golden {b}"


def _record(commit):
    """Write the golden file from the code in this checkout.  A case that
    raises (a fallback on the recording commit) is left out and reported."""
    cases, dropped = {}, {}
    for case in CASES:
        mp = pytest.MonkeyPatch()
        try:
            cases[case] = _trace(case, mp)
        except (RuntimeError, AssertionError) as e:
            dropped[case] = str(e)
        finally:
            mp.undo()
    GOLDEN.parent.mkdir(exist_ok=True)
    # one call per line, so a diff of the file reads as a diff of the trace
    body = ",\n".join(
        json.dumps(case) + ": [\n"
        + ",\n".join(json.dumps(c, separators=(",", ":")) for c in calls)
        + "\n]" for case, calls in cases.items())
    GOLDEN.write_text('{"recorded_from": ' + json.dumps(commit)
                      + ', "cases": {\n' + body + "\n}}\n")
    for case, calls in cases.items():
        print(f"{case}: {len(calls)} calls")
    for case, why in dropped.items():
        print(f"DROPPED {case}: {why}")


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        _record(sys.argv[2] if len(sys.argv) > 2 else "unknown")
    else:
        sys.exit(pytest.main([__file__, "-q", "-m", "gpu"]))
