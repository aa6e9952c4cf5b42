"""The fluid propagator's host side without a device: the C structs match their ctypes mirrors, the library and the
Python entry point refuse to run without a HIP device, and the pyapi_denise switch ``acoustic_kernels`` takes its two
values and refuses what the fluid kernels do not serve before any device work."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fluid_struct_layouts_match_header(tmp_path):
    """sizeof and every field offset of mifwi_fluid_desc / mifwi_fluid_layout as gcc lays out include/mifwi.h, against
    the ctypes mirrors (the method of test_abi.py)."""
    from physicsbasedfwi2_amd import _lib
    structs = {"mifwi_fluid_desc": _lib.FluidDesc, "mifwi_fluid_layout": _lib.FluidLayout}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mifwi.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append("return 0; }")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    assert ctypes.sizeof(_lib.FluidDesc) == 12 * 4
    assert [n for n, _ in _lib.FluidDesc._fields_] == ["nz", "nx", "nt", "nshot", "nsrc", "nrec", "ntap", "pml_width",
                                                       "free_surface", "shots_per_group", "source_type", "fd_order"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_fluid_has_no_cpu_fallback():
    from physicsbasedfwi2_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    d = _lib.FluidDesc(8, 8, 4, 1, 1, 1, 1, 0, 0, 0, 0, 4)
    rc = lib.mifwi_fluid_plan_create(ctypes.byref(h), 0, ctypes.byref(d))
    assert rc == -2 and b"no CPU fallback" in lib.mifwi_last_error()


def test_fluid_propagate_refuses_cpu_tensors():
    from physicsbasedfwi2_amd import fluid
    from physicsbasedfwi2_amd._lib import MifwiError
    with pytest.raises(MifwiError, match="HIP device"):
        fluid.propagate(torch.ones(3, 8, 8), torch.zeros(4, 1, 1), torch.zeros(6, 8), torch.zeros(6, 8),
                        torch.zeros(1, 1, 1, dtype=torch.int32), torch.ones(1, 1, 1),
                        torch.zeros(1, 1, 1, dtype=torch.int32), torch.ones(1, 1, 1), 0)


def test_fluid_materials_are_the_elastic_planes():
    """materials() = planes 0, 3, 4 of staggered_materials(vp, 0, rho), row 0 of K zeroed under a free surface
    (the torch definition; the device kernels are compared on the GPU)."""
    from physicsbasedfwi2_amd import elastic, fluid
    rng = np.random.default_rng(0)
    vp = torch.tensor(1500 + 1000 * rng.random((9, 11)), dtype=torch.float32)
    rho = torch.tensor(1000 + 1000 * rng.random((9, 11)), dtype=torch.float32)
    m5 = elastic.staggered_materials(vp, torch.zeros_like(vp), rho, 0.002, 20.0)
    assert torch.equal(m5[0], m5[1]) and not m5[2].any()
    m3 = fluid.materials(vp, rho, 0.002, 20.0)
    assert m3.shape == (3, 9, 11) and torch.equal(m3, m5[[0, 3, 4]])
    m3s = fluid.materials(vp, rho, 0.002, 20.0, free_surface=True)
    assert not m3s[0, 0].any() and torch.equal(m3s[0, 1:], m5[0, 1:]) and torch.equal(m3s[1:], m5[3:])


def _denise():
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    d = api.Denise("/nonexistent", verbose=0)
    d.ITERMAX, d.TIME, d.DT = 1, 0.1, 0.002
    vp = np.full((20, 30), 1500.0, dtype=np.float32)
    model = api.Model(vp, np.zeros_like(vp), np.full_like(vp, 1000.0), 20.0)
    src = api.Sources(np.array([300.0]), np.array([40.0]), 8.0)
    rec = api.Receivers(np.array([200.0, 400.0]), np.array([100.0, 100.0]))
    return api, d, model, src, rec


def test_shim_switch_values():
    api, d, *_ = _denise()
    assert d.acoustic_kernels == "elastic"
    d.acoustic_kernels = "fluid"
    assert d.acoustic_kernels == "fluid"
    d.acoustic_kernels = "elastic"
    for bad in ("acoustic", "Fluid", "", None, 1):
        with pytest.raises(api.MifwiError, match="acoustic_kernels"):
            d.acoustic_kernels = bad
    assert d.acoustic_kernels == "elastic"


def test_shim_refuses_what_the_fluid_kernels_do_not_serve(monkeypatch):
    """PHYSICS = 1 and EPRECOND != 0 with the fluid kernels raise before a device is touched: asking torch for one would
    raise something else here, or start the run."""
    api, d, model, src, rec = _denise()

    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the switch was checked")
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    d.acoustic_kernels = "fluid"
    d.PHYSICS = 1
    with pytest.raises(api.MifwiError, match="PHYSICS"):
        d.forward(model, src, rec)
    d.set_observed(np.zeros((1, 50, 2)), np.zeros((1, 50, 2)))
    with pytest.raises(api.MifwiError, match="PHYSICS"):
        d.grad(model, src, rec)
    d.PHYSICS, d.EPRECOND = 2, 1
    with pytest.raises(api.MifwiError, match="EPRECOND"):
        d.grad(model, src, rec)
    with pytest.raises(api.MifwiError, match="EPRECOND"):
        d.forward(model, src, rec)


def test_fuzz_draws_of_the_fluid_family_cover_what_they_are_meant_to():
    """The committed draws of test_fuzz_gpu.test_random_fluid_configuration: tile widths, nx % 4, source type x surface."""
    import test_fuzz_gpu
    test_fuzz_gpu.test_fluid_draws_cover_the_tile_widths_and_column_remainders()
