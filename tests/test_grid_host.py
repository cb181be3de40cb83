"""CPU test of the checks the three grid entry points share (csrc/caf_grid.h: grid_source, grid_sets_ok): one table of descriptors
and tables with exactly one fault each, run against caf_locate_grid, caf_locate_rtt and caf_crb_map.  Every pointer is a value
that is never dereferenced, so each call must be refused (or found empty) on the host.  The checks of each entry point's own
arguments are in test_locate_host.py, test_rtt_host.py and test_crb_host.py.  None needs a device."""

import ctypes as ct

import pytest

from pydsproutines_amd import _lib

FAKE = 4096  # never dereferenced: the refusals come first
POINTS = dict(source=_lib.CAF_LOCATE_POINTS, n=100, d_points=FAKE)
MESH = dict(source=_lib.CAF_LOCATE_MESH, ni=3, nj=4, d_a=FAKE, d_z=FAKE, d_c=FAKE, d_s=FAKE)
MESH_XY = dict(source=_lib.CAF_LOCATE_MESH_XY, ni=3, nj=4, d_a=FAKE, d_c=FAKE, z=50.0)  # (d_z and d_s are not read)
TABLE = dict(K=4, B=1, starts=None, records=FAKE)

# (what is wrong, the descriptor or None, the table)
FAULTS = [
    ("NULL descriptor", None, TABLE),
    ("unknown source", dict(POINTS, source=3), TABLE),
    ("n = 0", dict(POINTS, n=0), TABLE),
    ("NULL points", dict(POINTS, d_points=None), TABLE),
    ("ni = 0", dict(MESH, ni=0), TABLE),
    ("nj = -1", dict(MESH, nj=-1), TABLE),
    ("mesh: NULL d_a", dict(MESH, d_a=None), TABLE),
    ("mesh: NULL d_z", dict(MESH, d_z=None), TABLE),
    ("mesh: NULL d_c", dict(MESH, d_c=None), TABLE),
    ("mesh: NULL d_s", dict(MESH, d_s=None), TABLE),
    ("xy mesh: NULL d_a", dict(MESH_XY, d_a=None), TABLE),
    ("xy mesh: NULL d_c", dict(MESH_XY, d_c=None), TABLE),
    ("K = 0", POINTS, dict(TABLE, K=0)),
    ("cost_f32 = 2", dict(POINTS, cost_f32=2), TABLE),
    ("B = 0", POINTS, dict(TABLE, B=0)),
    ("B = 2 without offsets", POINTS, dict(TABLE, B=2)),
    ("B > K", POINTS, dict(TABLE, B=5, starts=FAKE)),
    ("B = 65536", POINTS, dict(TABLE, K=1 << 20, B=65536, starts=FAKE)),
    ("NULL records", POINTS, dict(TABLE, records=None)),
]


def descriptor(fields):
    d = _lib.CafLocateDesc()
    d.mode = _lib.CAF_LOCATE_TD  # (read by caf_locate_grid alone)
    for name, v in fields.items():
        setattr(d, name, v)
    return d


def ptr(v):
    return None if v is None else ct.c_void_p(v)


def locate_grid(lib, desc, t, out):
    return lib.caf_locate_grid(desc, ptr(t["records"]), t["K"], ptr(t["starts"]), t["B"], ptr(out), None, None, None)


def locate_rtt(lib, desc, t, out):
    return lib.caf_locate_rtt(desc, ptr(t["records"]), t["K"], ptr(t["starts"]), t["B"], 0, ptr(out), None, None, None)


def crb_map(lib, desc, t, out):
    return lib.caf_crb_map(desc, ptr(t["records"]), t["K"], ptr(t["starts"]), t["B"], _lib.CAF_CRB_RADIAL, None, None, None, ptr(out),
                           None, None, None, None, None)


ENTRIES = {"caf_locate_grid": locate_grid, "caf_locate_rtt": locate_rtt, "caf_crb_map": crb_map}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_single_fault_is_refused_in_the_entry_points_name(entry):
    lib = _lib.load()
    for what, fields, table in FAULTS:
        desc = ct.byref(descriptor(fields)) if fields is not None else None
        assert ENTRIES[entry](lib, desc, table, FAKE) == _lib.CAF_ERR_INVALID, what
        assert _lib.last_error().startswith(entry + ": "), (what, _lib.last_error())


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_nothing_asked_for_is_an_empty_job_for_each_source(entry):
    lib = _lib.load()
    for fields in (POINTS, MESH, MESH_XY):
        assert ENTRIES[entry](lib, ct.byref(descriptor(fields)), TABLE, None) == _lib.CAF_OK, fields["source"]
