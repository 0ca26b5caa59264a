"""The ctypes signatures come from include/lrm.h alone (lrm_amd._capi.parse_header): the parser on hand-made header text, on
the real header, a few prototypes spelled out by hand where a miscount or a wrong type code would show, and the property the
hand-written table of earlier versions could not give: after load() EVERY declared function the library exports has its
argtypes and restype set from its prototype."""
import ctypes as C

import pytest

VP, SZ, FP = C.c_void_p, C.c_size_t, C.c_float


@pytest.fixture(scope="module")
def capi(lrm):
    from lrm_amd import _capi
    return _capi


def test_comment_inside_a_parameter_list(capi):
    text = "int lrm_a(const float* quats /* device, nposes x 4 */, size_t nposes, // trailing, with a comma\n void* ws);"
    assert capi.parse_header(text) == {"lrm_a": (C.c_int, [VP, SZ, VP])}


def test_array_parameters_are_pointers(capi):
    text = "void lrm_rot(const float quat[4], const LrmLegDimensions* leg);\nint lrm_counts(uint64_t out[4]);"
    assert capi.parse_header(text) == {"lrm_rot": (None, [VP, VP]), "lrm_counts": (C.c_int, [VP])}


def test_void_parameter_list(capi):
    assert capi.parse_header("int lrm_device_count(void);") == {"lrm_device_count": (C.c_int, [])}


def test_prototype_over_three_lines_between_preprocessor_lines(capi):
    text = "#define LRM_X 8\nint lrm_b(const float* x,\n          size_t n, float margin,\n          void* stream);\n#ifdef __cplusplus\n}\n#endif\n"
    assert capi.parse_header(text) == {"lrm_b": (C.c_int, [VP, SZ, FP, VP])}


def test_the_callback_typedef_is_no_prototype_and_its_type_is_a_pointer(capi):
    typedef = "typedef int (*LrmOctExchange)(uint32_t* flags, size_t n, void* user);\n"
    assert capi.parse_header(typedef) == {}
    text = typedef + "int lrm_oct(const float* f, size_t n, int rank, int world, LrmOctExchange exchange, void* user);"
    assert capi.parse_header(text) == {"lrm_oct": (C.c_int, [VP, SZ, C.c_int, C.c_int, VP, VP])}


def test_struct_typedefs_are_no_prototypes(capi):
    text = "typedef struct LrmS {\n    float a;\n    int32_t lrm_like[3];\n} LrmS;\nvoid lrm_s(LrmS* out);"
    assert capi.parse_header(text) == {"lrm_s": (None, [VP])}


@pytest.mark.parametrize("ret, want", [("int", C.c_int), ("size_t", C.c_size_t), ("void", None), ("const char*", C.c_char_p),
                                       ("const char *", C.c_char_p)])
def test_return_types(capi, ret, want):
    assert capi.parse_header(f"{ret} lrm_r(void);") == {"lrm_r": (want, [])}


def test_scalars_by_value(capi):
    text = "int lrm_v(uint8_t links, uint32_t skip, uint64_t w, int32_t i, int fn, double d, float f, size_t n, const float g);"
    assert capi.parse_header(text)["lrm_v"][1] == [C.c_uint8, C.c_uint32, C.c_uint64, C.c_int32, C.c_int, C.c_double, FP, SZ, FP]


@pytest.mark.parametrize("text", ["int lrm_u(unsigned n);", "int lrm_u(long n);", "int lrm_u(LrmLegDimensions leg);",
                                  "float lrm_u(void);", "unsigned int lrm_u(void);", "int lrm_u();"])
def test_an_unknown_type_raises_and_names_the_function(capi, text):
    with pytest.raises(capi.LrmError, match="lrm_u"):
        capi.parse_header(text)


def test_real_header(lrm, capi):
    sigs = capi.parse_header(open(capi.HEADER_PATH).read())
    assert sigs == capi.signatures() and sigs
    assert lrm.declared_symbols() == sorted(sigs) and len(lrm.declared_symbols()) == len(sigs)
    assert "lrm_get_M2_leg" in sigs  # the one name a lower-case pattern misses
    assert set(lrm.declared_symbols()) <= set(lrm.exported_symbols())


def test_a_missing_header_is_an_error_with_its_path(capi, monkeypatch, tmp_path):
    monkeypatch.setattr(capi, "_signatures", None)
    monkeypatch.setattr(capi, "HEADER_PATH", str(tmp_path / "include" / "lrm.h"))
    with pytest.raises(capi.LrmError, match="lrm.h"):
        capi.signatures()


def test_spot_checks_written_from_the_header(capi):
    sigs = capi.signatures()
    trunk = sigs["lrm_trunk_clearance_posed_dev"]
    assert trunk == (C.c_int, [VP, VP, SZ, SZ, VP, SZ, VP, VP, VP, VP, FP, FP, FP, FP, FP, C.c_uint8, VP, VP, VP, VP, VP, VP])
    assert len(trunk[1]) == 22
    swing = sigs["lrm_swing_transit_posed_dev"]
    assert swing == (C.c_int, [VP, VP, VP, SZ, VP, VP, SZ, VP, SZ, VP, VP, SZ, VP, VP, SZ, FP, VP, FP, FP, C.c_uint32] + [VP] * 13)
    assert len(swing[1]) == 33
    assert sigs["lrm_dbg_exact_math_sums_host"] == (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, VP])
    assert sigs["lrm_apply_oct_dev"] == (C.c_int, [VP, VP, VP, SZ, VP, VP, VP, SZ, VP, VP, C.c_int, C.c_int, VP, VP])
    assert sigs["lrm_leg_factory"] == (None, [FP] * 11 + [VP])
    assert sigs["lrm_posed_workspace_bytes"] == (SZ, [SZ, SZ])
    assert sigs["lrm_version"] == (C.c_char_p, [])


def test_every_exported_function_is_typed_after_load(lrm, capi):
    L = lrm.load()
    exported = set(lrm.exported_symbols())
    typed = 0
    for name, (restype, argtypes) in capi.signatures().items():
        if name not in exported:
            continue
        fn = getattr(L, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name
        assert fn.restype is restype, name
        typed += 1
    assert typed == len(capi.signatures())  # this build exports everything the header declares
    assert isinstance(L.lrm_version(), bytes) and isinstance(L.lrm_posed_workspace_bytes(1, 1), int)
