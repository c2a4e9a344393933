"""Completion of the synchronous DFT_ComputeXC without a publishing kernel (option "publish", csrc/dft_api.hip): the
reduce kernel's finishing block stores Exc to the host word and a stream memory write behind it raises a per-call
sequence word.  Both forms (0 = k_publish_exc, 1 = stream write) in one process: same bits, same completion contract
(the call has returned = every store of the call is visible to any stream), same error text.  Where the creation-time
probe fell back to the kernel the publish = 1 cases skip and say so."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)
import quantum_compute_dft_amd as q  # noqa: E402
from helpers import synth_inputs  # noqa: E402

XC = {"LDA": 0, "GGA": 1, "B3LYP": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _solver(name, publish, **opts):
    s = q.DFTSolverWrapper(q.build_library(), name)
    s.set_option("graph", 0)          # a recorded sweep keeps the publishing kernel: plain launches are what is under test
    s.set_option("publish", publish)
    for k, v in opts.items():
        s.set_option(k, v)
    if publish == 1 and s.get_option("publish_probe") != 1.0:
        pytest.skip("the runtime refused the stream memory write at solver creation: the solver fell back to k_publish_exc")
    assert s.get_option("publish_live") == float(publish)
    return s


def _dev_inputs(name, nao, ngrid, dev, seed=11):
    dm, ao, gr, w = synth_inputs(ngrid, nao, need_grad=name != "LDA", seed=seed)
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return (dm, ao, gr, w), (t(dm), t(ao), t(gr), t(w))


@pytest.fixture(scope="module")
def gga114(dev):
    """(GGA, 114, 1000): host inputs, device inputs and the oracle's numbers, shared and left unchanged."""
    host, devs = _dev_inputs("GGA", 114, 1000, dev)
    dm, ao, gr, w = host
    return host, devs, oracle.compute_xc(1, dm, ao, w, gr)


def test_option_defaults_and_read_back(dev):
    s = q.DFTSolverWrapper(q.build_library(), "GGA")
    assert s.get_option("publish") == -1.0                                   # auto ...
    assert s.get_option("publish_live") == 0.0                               # ... is the kernel: the stream write measured slower
    s.set_option("publish", 1)
    assert s.get_option("publish_live") == s.get_option("publish_probe")    # asked for: live where the probe passed
    s.set_option("publish", 0)
    assert s.get_option("publish") == 0.0 and s.get_option("publish_live") == 0.0
    with pytest.raises(KeyError):
        s.get_option("no_such_option")


@pytest.mark.parametrize("name,nao,ngrid,tiny", [("GGA", 114, 1000, 0), ("LDA", 24, 777, 1), ("B3LYP", 40, 300, 0)])
def test_both_forms_return_the_same_bits(dev, name, nao, ngrid, tiny):
    host, (d_dm, d_ao, d_gr, d_w) = _dev_inputs(name, nao, ngrid, dev)
    out = {}
    for publish in (0, 1):
        s = _solver(name, publish, tiny=tiny, profile=1)
        d_v = torch.full((nao, nao), 7.0, dtype=torch.float64, device=dev)
        exc = s.compute_xc(ngrid, nao, d_dm, d_ao, d_w, d_v, d_gr)
        assert s.get_option("used_publish") == float(publish)
        assert ("sweep_tiny" in [n for n, _ in s.timings()]) == bool(tiny)   # the path under test is the one that ran
        torch.cuda.synchronize()
        out[publish] = (exc, d_v.cpu().numpy())
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1])
    exc_ref, v_ref = oracle.compute_xc(XC[name], *[host[i] for i in (0, 1, 3, 2)])
    assert out[1][0] == pytest.approx(exc_ref, rel=1e-12, abs=1e-14)
    assert np.abs(out[1][1] - v_ref).max() <= 1e-11 * np.abs(v_ref).max() + 1e-13


@pytest.mark.parametrize("publish", [0, 1])
def test_each_of_200_calls_returns_its_own_exc(dev, gga114, publish):
    """Back to back, a differently scaled dm each call: a call that returned on a stale word (the previous call's Exc or
    sequence number) would hand back the wrong energy.  Expected values: the asynchronous entry on the same inputs."""
    _, (d_dm, d_ao, d_gr, d_w), _ = gga114
    nao, ngrid, ncall = 114, 1000, 200
    scale = 1.0 + 0.01 * torch.arange(ncall, dtype=torch.float64, device=dev)
    dms = (scale[:, None, None] * d_dm[None]).contiguous()
    d_v = torch.zeros((nao, nao), dtype=torch.float64, device=dev)
    s = _solver("GGA", publish)
    d_exc = torch.zeros(ncall, dtype=torch.float64, device=dev)
    for k in range(ncall):
        s.compute_xc_async(ngrid, nao, dms[k], d_ao, d_w, d_v, d_exc[k:], d_gr)
    torch.cuda.synchronize()
    want = d_exc.cpu().numpy()
    assert len(set(want.tolist())) == ncall          # the inputs really differ call by call
    got = np.array([s.compute_xc(ngrid, nao, dms[k], d_ao, d_w, d_v, d_gr) for k in range(ncall)])
    assert s.get_option("used_publish") == float(publish)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("publish", [0, 1])
def test_vxc_is_visible_to_another_stream_when_the_call_returns(dev, gga114, publish, own_stream):
    """No synchronise between the call's return and a copy of d_vxc queued on a DIFFERENT (non-blocking) stream."""
    _, (d_dm, d_ao, d_gr, d_w), (exc_ref, v_ref) = gga114
    nao, ngrid = 114, 1000
    s = _solver("GGA", publish)
    run = torch.cuda.Stream(device=dev) if own_stream else None
    if run is not None:
        s.set_stream(run.cuda_stream)
    other = torch.cuda.Stream(device=dev)
    d_v = torch.empty((nao, nao), dtype=torch.float64, device=dev)
    copies = []
    for _ in range(20):
        d_v.fill_(7.0)
        torch.cuda.synchronize()
        exc = s.compute_xc(ngrid, nao, d_dm, d_ao, d_w, d_v, d_gr)
        with torch.cuda.stream(other):
            copies.append(d_v.clone())
        assert exc == pytest.approx(exc_ref, rel=1e-12, abs=1e-14)
    other.synchronize()
    for c in copies:
        assert np.abs(c.cpu().numpy() - v_ref).max() <= 1e-11 * np.abs(v_ref).max() + 1e-13
    torch.cuda.synchronize()
    s.set_stream(0)


@pytest.mark.parametrize("publish", [0, 1])
def test_non_finite_input_still_reports_the_nan_error(dev, gga114, publish):
    _, (d_dm, d_ao, d_gr, d_w), (exc_ref, _) = gga114
    nao, ngrid = 114, 1000
    bad = d_ao.clone()
    bad[3, 5] = float("nan")
    s = _solver("GGA", publish)
    d_v = torch.zeros((nao, nao), dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="Exc is NaN after the sweep completed"):
        s.compute_xc(ngrid, nao, d_dm, bad, d_w, d_v, d_gr)
    # and the solver is fine afterwards
    assert s.compute_xc(ngrid, nao, d_dm, d_ao, d_w, d_v, d_gr) == pytest.approx(exc_ref, rel=1e-12, abs=1e-14)
