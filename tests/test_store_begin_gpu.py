"""mpg_regrid_store_begin / mpg_regrid_store_grid_begin (round 6): the independent RegridStores of a run (interp.F90:123, 207-437 stores
them one after the other) started on the library's worker thread and collected by the plain calls.  The bar: the SAME weights, bit for
bit, whatever runs beside the worker; cache / reference-count behaviour of the plain calls; nothing left behind."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _weights(rh):
    if rh.nnz_per_row == 0:        # conservative: CSR
        return rh.csr()
    return rh.weights()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_begun_stores_give_the_plain_calls_weights(gpu_lib, regional_case):
    from mpassit_amd import regrid as R
    m, g = regional_case
    mesh_a, grid_a = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    mesh_b, grid_b = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    specs = [(R.REGRIDMETHOD_BILINEAR, R.MESHLOC_ELEMENT), (R.REGRIDMETHOD_CONSERVE, R.MESHLOC_ELEMENT), (R.REGRIDMETHOD_NEAREST_STOD, R.MESHLOC_ELEMENT),
             (R.REGRIDMETHOD_BILINEAR, R.MESHLOC_NODE)]
    for method, loc in specs:                       # all queued before any is collected
        R.regrid_store_begin(mesh_a, grid_a, method, meshloc=loc)
    for st in (R.STAGGERLOC_EDGE1, R.STAGGERLOC_EDGE2):
        R.regrid_store_grid_begin(grid_a, st)
    for method, loc in specs:
        ra, rb = R.regrid_store(mesh_a, grid_a, method, meshloc=loc), R.regrid_store(mesh_b, grid_b, method, meshloc=loc)
        assert _same(_weights(ra), _weights(rb)), (method, loc)
        assert ra.store_ms > 0
        ra.release()
        rb.release()
    for st in (R.STAGGERLOC_EDGE1, R.STAGGERLOC_EDGE2):
        ra, rb = R.regrid_store_grid(grid_a, st), R.regrid_store_grid(grid_b, st)
        assert _same(ra.weights(), rb.weights())
        ra.release()
        rb.release()
    for o in (mesh_a, mesh_b, grid_a, grid_b):
        o.destroy()


def test_cache_and_refcount_behave_as_for_plain_stores(gpu_lib, regional_case):
    from mpassit_amd import regrid as R
    m, g = regional_case
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD)
    R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD)            # already queued / running / cached: nothing new
    a = R.regrid_store(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD)
    b = R.regrid_store(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD)
    assert a._h.value == b._h.value                                          # one weight set, two references
    t = a.store_ms
    a.release()
    b.release()
    R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD)            # parked in the cache: no second Store
    c = R.regrid_store(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD)
    assert c.store_ms == t
    c.release()
    # begun, never collected, and the mesh goes away while the worker may still be at it: destroy waits for the worker
    R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_CONSERVE)
    mesh.destroy()
    grid.destroy()


def _begun_stores_and_a_window(m, g, serial):
    """Two begun Stores on (mesh, grid), a windowed mesh cut to the same grid at once, three Stores on it, then the two collected.
    serial: mpg_warmup_wait (which drains the worker) after every call."""
    from mpassit_amd import _lib as L, regrid as R

    def step(x=None):
        if serial:
            L.check(L.load().mpg_warmup_wait())
        return x
    mesh, grid = step(R.Mesh.from_mpas(m)), step(R.Grid.from_target(g))
    step(R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_CONSERVE))
    step(R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_BILINEAR))
    wmesh = step(R.Mesh.from_mpas(m, window_grid=grid))
    got = [wmesh.window_info()]
    handles = []
    for o, method in ((wmesh, R.REGRIDMETHOD_BILINEAR), (wmesh, R.REGRIDMETHOD_NEAREST_STOD), (wmesh, R.REGRIDMETHOD_CONSERVE),
                      (mesh, R.REGRIDMETHOD_CONSERVE), (mesh, R.REGRIDMETHOD_BILINEAR)):
        handles.append(step(R.regrid_store(o, grid, method)))
        got.append([np.array(a) for a in _weights(handles[-1])])
    for rh in handles:
        rh.release()
    for o in (wmesh, mesh, grid):
        o.destroy()
    return got


def test_begun_stores_and_a_window_on_one_grid(gpu_lib, regional_case):
    """mpg_mesh_create_window builds the grid's point and cell pyramids on the caller's thread; a begun Store on that grid builds them on
    the worker.  The call drains the worker first, so the window and all five weight sets are those of the same calls made one after
    the other.  A guard that must pass: without the drain the two threads race, and a race cannot be made to fail on demand."""
    m, g = regional_case
    want = _begun_stores_and_a_window(m, g, serial=True)
    got = _begun_stores_and_a_window(m, g, serial=False)
    assert got[0] == want[0] and 0 < got[0][1] <= m.nCells
    assert len(got) == len(want) == 6
    for a, b in zip(got[1:], want[1:]):
        assert len(a) == len(b) >= 2 and _same(a, b)


def test_one_handle_per_distinct_store(gpu_lib):
    """Every Store entry point on one mesh pair and one projection-built grid (the periodic Store, which refuses that regional grid, on a
    small global one): the same call twice returns the same handle, every distinct call a handle of its own.  The line type in force is
    part of a bilinear handle and of no other."""
    import _mesh_to_mesh_cases as MC
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    BIL, CON, NN = R.REGRIDMETHOD_BILINEAR, R.REGRIDMETHOD_CONSERVE, R.REGRIDMETHOD_NEAREST_STOD
    a, b = R.Mesh.from_mpas(MC.mesh("geo8")), R.Mesh.from_mpas(MC.mesh("vor1500"))
    grid = R.Grid.from_proj(tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, ref_lat=38.5, ref_lon=-97.5, truelat1=38.5,
                                                         truelat2=38.5, stand_lon=-97.5), fill_target=False)
    globe = R.Grid.from_target(tg.define_target_grid_params("lat-lon", nx=24, ny=12, stand_lon=0.0, is_regional=False))
    calls = [lambda m=m, loc=loc, st=st: R.regrid_store(a, grid, m, staggerloc=st, meshloc=loc)
             for m, loc, st in ((BIL, R.MESHLOC_ELEMENT, R.STAGGERLOC_CENTER), (BIL, R.MESHLOC_NODE, R.STAGGERLOC_CENTER),
                                (BIL, R.MESHLOC_ELEMENT, R.STAGGERLOC_EDGE1), (NN, R.MESHLOC_ELEMENT, R.STAGGERLOC_CENTER),
                                (CON, R.MESHLOC_ELEMENT, R.STAGGERLOC_CENTER))]
    calls += [lambda: R.regrid_store(b, grid, BIL)]
    calls += [lambda st=st: R.regrid_store_grid(grid, st) for st in (R.STAGGERLOC_EDGE1, R.STAGGERLOC_EDGE2)]
    calls += [lambda m=m, loc=loc, st=st: R.regrid_store_to_mesh(grid, a, m, staggerloc=st, meshloc=loc)
              for m, loc, st in ((BIL, R.MESHLOC_ELEMENT, R.STAGGERLOC_CENTER), (NN, R.MESHLOC_ELEMENT, R.STAGGERLOC_CENTER),
                                 (BIL, R.MESHLOC_NODE, R.STAGGERLOC_CENTER), (BIL, R.MESHLOC_ELEMENT, R.STAGGERLOC_CORNER))]
    calls += [lambda p=p: R.regrid_store_periodic_to_mesh(globe, a, pole_method=p) for p in (R.POLEMETHOD_ALLAVG, R.POLEMETHOD_NONE)]
    calls += [lambda n=n: R.regrid_store_conserve_to_mesh(grid, a, norm=n) for n in (R.NORM_DSTAREA, R.NORM_FRACAREA)]
    calls += [lambda m=m, loc=loc: R.regrid_store_mesh(a, b, m, dst_meshloc=loc)
              for m, loc in ((BIL, R.MESHLOC_ELEMENT), (NN, R.MESHLOC_ELEMENT), (BIL, R.MESHLOC_NODE))]
    calls += [lambda: R.regrid_store_mesh(b, a, BIL)]
    calls += [lambda n=n: R.regrid_store_conserve_mesh(a, b, norm=n) for n in (R.NORM_DSTAREA, R.NORM_FRACAREA)]
    held = []
    try:
        R.regrid_store_begin(a, grid, CON)                      # the two _begin forms: the plain calls below collect their handles
        R.regrid_store_grid_begin(grid, R.STAGGERLOC_EDGE2)
        first = [c() for c in calls]
        held += first
        again = [c() for c in calls]
        held += again
        assert [h._h.value for h in first] == [h._h.value for h in again]
        assert len({h._h.value for h in first}) == len(calls) == 22
        # the line type: nearest Stores share their handle across it, bilinear ones do not
        L.tune("bilinear_linetype", 1)
        held += [R.regrid_store(a, grid, NN), R.regrid_store_mesh(a, b, NN), R.regrid_store(a, grid, CON), R.regrid_store(a, grid, BIL),
                 R.regrid_store_mesh(a, b, BIL)]
        assert [h._h.value for h in held[-5:-2]] == [first[3]._h.value, first[17]._h.value, first[4]._h.value]
        assert not {h._h.value for h in held[-2:]} & {h._h.value for h in first} and held[-2]._h.value != held[-1]._h.value
        L.tune("bilinear_linetype", 0)
        held += [R.regrid_store(a, grid, BIL), R.regrid_store_mesh(a, b, BIL)]
        assert [h._h.value for h in held[-2:]] == [first[0]._h.value, first[16]._h.value]
    finally:
        L.tune("bilinear_linetype", 0)
        for h in held:
            h.release()
        for o in (a, b, grid, globe):
            o.destroy()


def test_refused_arguments_are_refused_at_once(gpu_lib, regional_case):
    from mpassit_amd import _lib as L, regrid as R
    m, g = regional_case
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    with pytest.raises(L.MpgError):
        R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_CONSERVE, staggerloc=R.STAGGERLOC_EDGE1)
    with pytest.raises(L.MpgError):
        R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD, meshloc=R.MESHLOC_NODE)
    with pytest.raises(L.MpgError):
        R.regrid_store_grid_begin(grid, R.STAGGERLOC_CENTER)
    mesh.destroy()
    grid.destroy()


def test_regrids_beside_the_worker_and_interp_data_either_way(gpu_lib, global_mesh, conus_grid_30km):
    """The caller's thread regrids on its own stream while the worker builds the other weight sets; then the whole interp_data with
    and without the overlap: every output bit for bit."""
    import torch
    from mpassit_amd import interp as I, regrid as R
    m, g = global_mesh, conus_grid_30km
    nz = 8
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    src = torch.rand((nz, m.nCells), dtype=torch.float64, device="cuda", generator=gen)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    want = rh.regrid(src.view(-1), nlev=nz).clone()
    torch.cuda.synchronize()
    R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_CONSERVE)
    R.regrid_store_begin(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD)
    R.regrid_store_grid_begin(grid, R.STAGGERLOC_EDGE2)
    for _ in range(20):
        got = rh.regrid(src.view(-1), nlev=nz)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    rh.release()
    mesh.destroy()
    grid.destroy()

    inp = I.InputData(nz=nz, nzp1=nz + 1, nsoil=4, hgt=torch.rand(m.nCells, dtype=torch.float64, device="cuda", generator=gen))
    hist2 = [("skintemp", "TSK"), ("snow", "SNOW"), ("xland", "XLAND")]
    hist3 = [("uReconstructZonal", "U"), ("uReconstructMeridional", "V"), ("theta", "T"), ("w", "W")]
    soil = [("smois", "SMOIS")]
    for n, _ in hist2:
        inp.hist[n] = torch.floor(torch.rand(m.nCells, dtype=torch.float64, device="cuda", generator=gen) * 3)
    for n, _ in hist3:
        inp.hist[n] = torch.rand((nz + 1 if n == "w" else nz, m.nCells), dtype=torch.float64, device="cuda", generator=gen)
    inp.hist["smois"] = torch.rand((4, m.nCells), dtype=torch.float64, device="cuda", generator=gen)
    outs = {}
    for overlap in (True, False):
        mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)          # fresh objects: every Store really runs
        cfg = I.InterpConfig(interp_diag=False, wrf_mod_vars=True, hist_2d=hist2, hist_3d=hist3, hist_soil=soil, overlap_stores=overlap)
        outs[overlap] = {k: v.clone() for k, v in I.interp_data(mesh, grid, g, inp, cfg).items()}
        torch.cuda.synchronize()
        mesh.destroy()
        grid.destroy()
    assert set(outs[True]) == set(outs[False]) and len(outs[True]) >= 8
    for k in outs[True]:
        assert torch.equal(outs[True][k], outs[False][k]), k
