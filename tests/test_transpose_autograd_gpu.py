"""regrid.regrid_autograd / regrid.RegridFunction: the Regrid as a differentiable torch op whose backward is the transpose Regrid,
and the transpose captured in a torch.cuda graph."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(gpu_lib):
    """A bilinear handle small enough for gradcheck's dense Jacobians."""
    from mpassit_amd import regrid as R, synth, target_grid as T
    m = synth.global_voronoi_mesh(400)
    t = T.define_target_grid_params("lat-lon", nx=13, ny=9, stand_lon=0.0, is_regional=False)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(t)
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    yield rh
    rh.release()
    mesh.destroy()
    grid.destroy()


@pytest.mark.parametrize("layout", [0, 1])
def test_gradcheck(small, layout):
    import torch
    from mpassit_amd import regrid as R
    rh, nlev, nf = small, 2, 2
    shape = (nf, nlev, rh.n_src) if layout == R.LAYOUT_CELL_FAST else (nf, rh.n_src, nlev)
    x = torch.randn(shape, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3), requires_grad=True)
    assert torch.autograd.gradcheck(lambda s: R.regrid_autograd(rh, s, nlev=nlev, nfields=nf, layout=layout), (x,), eps=1e-6, atol=1e-9)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("layout", [0, 1])
def test_backward_is_regrid_transpose(small, layout, dtype):
    import torch
    from mpassit_amd import regrid as R
    rh, nlev = small, 3
    dt = getattr(torch, dtype)
    shape = (nlev, rh.n_src) if layout == R.LAYOUT_CELL_FAST else (rh.n_src, nlev)
    x = torch.randn(shape, dtype=torch.float64, device="cuda").to(dt).requires_grad_()
    y = R.regrid_autograd(rh, x, nlev=nlev, layout=layout)
    assert y.dtype == dt and tuple(y.shape) == (1, nlev, rh.ny_dst, rh.nx_dst)
    assert torch.equal(y, rh.regrid_typed(x.detach(), nlev=nlev, layout=layout))
    gy = torch.randn(y.shape, dtype=torch.float64, device="cuda").to(dt)
    y.backward(gy)
    want = rh.regrid_transpose(gy, nlev=nlev, layout=layout, out_dtype=dt).reshape(shape)
    assert x.grad.dtype == dt and torch.equal(x.grad, want)


def test_transpose_replays_in_a_graph(small):
    import torch
    rh, nlev = small, 4
    g = torch.randn((1, nlev, rh.n_dst), dtype=torch.float64, device="cuda")
    out = torch.empty((1, nlev, rh.n_src), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rh.regrid_transpose(g, nlev=nlev, out=out)          # warm-up: builds the transposed index (allocates, synchronises)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = out.clone()
    out.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rh.regrid_transpose(g, nlev=nlev, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    g.mul_(-2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, -2.0 * eager)
