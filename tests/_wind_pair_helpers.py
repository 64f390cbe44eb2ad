"""What the GPU tests of the two wind calls on a pair of fixed handles share (test_wind_to_mesh_gpu.py, test_wind_to_edges_gpu.py): the
either-handle unmapped mask, the comparison of two tensors as integers, random winds on the handles' sources and plane-pitched NaN-filled
views."""


def _unmapped(torch, rh_u, rh_v):
    """the points either handle leaves unmapped, as a CUDA mask"""
    un = (rh_u.weights()[0][:, 0] < 0) | (rh_v.weights()[0][:, 0] < 0)
    return torch.as_tensor(un, device="cuda")


def _bytes_equal(a, b):
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = torch.int64 if a.dtype == torch.float64 else torch.int32       # compared as integers: -0.0 is not +0.0, NaN equals itself
    return torch.equal(a.contiguous().reshape(-1).view(bits), b.contiguous().reshape(-1).view(bits))


def _winds(torch, rh_u, rh_v, nlev, sdt, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    u = (torch.randn((nlev, rh_u.n_src), dtype=torch.float64, device="cuda", generator=gen) * 12.0).to(sdt)
    v = (torch.randn((nlev, rh_v.n_src), dtype=torch.float64, device="cuda", generator=gen) * 12.0).to(sdt)
    return u, v


def _pitched(torch, nlev, ny, nx, dt, ld):
    """a NaN-filled buffer and its (nlev, ny, nx) view with level planes ld elements apart (RouteHandle.empty_pitched with a given stride)"""
    buf = torch.full((nlev * ld,), float("nan"), dtype=dt, device="cuda")
    return buf, buf.as_strided((nlev, ny, nx), (ld, nx, 1))
