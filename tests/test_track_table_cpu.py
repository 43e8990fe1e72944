"""The device-resident track table's entries (cvhip_tracks_*) without a GPU: the library exports them, and
cvhip_tracks_create's argument checks and cvhip_tracks_destroy(NULL) touch no device."""
import ctypes as C

from cybervision_amd import _lib, build

SYMBOLS = ["cvhip_tracks_create", "cvhip_tracks_destroy", "cvhip_tracks_info", "cvhip_tracks_assign", "cvhip_tracks_read",
           "cvhip_tracks_extend", "cvhip_tracks_merge", "cvhip_tracks_select_columns", "cvhip_tracks_gather"]
INVALID = -1  # CVHIP_ERR_INVALID


def test_library_exports_the_track_table_entries():
    build.build()
    L = C.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES


def test_create_checks_its_arguments_without_a_device():
    L = _lib.lib()
    out = C.c_void_p()
    not_a_device = C.c_void_p(0x1000)  # never dereferenced: m = 0 and the NULL output are refused first
    assert L.cvhip_tracks_create(None, 3, 0, C.byref(out)) == INVALID
    assert L.cvhip_tracks_create(None, 0, 0, None) == INVALID
    assert L.cvhip_tracks_create(not_a_device, 3, 0, None) == INVALID
    assert L.cvhip_tracks_create(not_a_device, 0, 16, C.byref(out)) == INVALID
    assert not out.value
    assert b"m = 0" in L.cvhip_last_error()


def test_destroy_null_is_a_no_op():
    assert _lib.lib().cvhip_tracks_destroy(None) is None


def test_python_layer_has_the_resident_switch():
    import inspect

    from cybervision_amd import reconstruction, triangulation

    assert hasattr(triangulation, "DeviceTrackTable")
    for fn in (reconstruction.reconstruct_perspective, reconstruction.reconstruct_perspective_surface,
               triangulation.PerspectiveTriangulation.__init__):
        assert inspect.signature(fn).parameters["resident_tracks"].default is False
