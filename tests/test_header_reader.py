"""manhattanslam_amd/_header.py, the reader the Python binding is built from, on a few lines of synthetic header text each: what it does not know
it refuses by name, and what it reads has C's layout.  (The real headers against a compiler: tests/test_abi.py.)  No GPU needed."""
import ctypes as C

import pytest


def H():
    from manhattanslam_amd import _header
    return _header


def test_unknown_scalar_type_is_refused_not_defaulted():
    decl = H().declarations("MSL_API int msl_f(int n, short x) MSL_NOEXCEPT;")
    assert decl == {"msl_f": ("int", [("int", "n"), ("short", "x")])}
    with pytest.raises(H().MslError, match="msl_f: parameter x.*short"):
        H().ctypes_of(decl["msl_f"], "msl_f")
    with pytest.raises(H().MslError, match="msl_g: return value.*uint64_t"):
        H().ctypes_of(H().declarations("MSL_API uint64_t msl_g(void) MSL_NOEXCEPT;")["msl_g"], "msl_g")


def test_function_pointer_parameter_is_refused():
    with pytest.raises(H().MslError, match=r"msl_f: .*\(\*cb\)"):
        H().declarations("MSL_API int msl_f(void (*cb)(int, float), int n) MSL_NOEXCEPT;")


def test_statement_without_noexcept_is_refused():
    with pytest.raises(H().MslError, match="msl_second"):
        H().declarations("MSL_API int msl_first(void) MSL_NOEXCEPT;\nMSL_API int msl_second(int n);\n")
    with pytest.raises(H().MslError, match="msl_first"):                                    # a lost `;` swallows the next statement
        H().declarations("MSL_API int msl_first(void)\nMSL_API int msl_second(int n) MSL_NOEXCEPT;\n")
    with pytest.raises(H().MslError, match="2 MSL_API tokens but 1"):                       # one name declared twice
        H().declarations("MSL_API int msl_first(void) MSL_NOEXCEPT;\nMSL_API int msl_first(int n) MSL_NOEXCEPT;\n")


def test_field_of_an_undeclared_record_is_refused():
    with pytest.raises(H().MslError, match="msl_a: .*msl_later"):
        H().records("typedef struct msl_a { float x; msl_later inner; } msl_a;\ntypedef struct msl_later { float y; } msl_later;")
    with pytest.raises(H().MslError, match="msl_a: .*v"):
        H().records("typedef struct msl_a { float v[MSL_UNDEFINED]; } msl_a;")


def test_colliding_flattened_members_are_refused():
    with pytest.raises(H().MslError, match=r"msl_b: .*\['x'\]"):
        H().records("typedef struct msl_a { float x, y; } msl_a;\ntypedef struct msl_b { msl_a base; int32_t x; } msl_b;")


def test_comments_are_not_read(tmp_path, monkeypatch):
    monkeypatch.setattr(H(), "INCLUDE", str(tmp_path))
    (tmp_path / "x.h").write_text("/* MSL_API int msl_old(int n);\n * gone */\n// MSL_API int msl_older(void);\n#define MSL_API\n"
                                  "MSL_API const char *msl_name(int k /* MSL_API; */) MSL_NOEXCEPT;\n")
    src = H().text("x.h")
    assert "msl_old" not in src and H().declarations(src) == {"msl_name": ("const char *", [("int", "k")])}
    with pytest.raises(H().MslError, match=str(tmp_path / "y.h")):
        H().text("y.h")


def test_ctypes_rules():
    decl = H().declarations("MSL_API void msl_f(const float pose[16], int32_t *out, const char *path, msl_mem mem, unsigned flags, size_t n,\n"
                            "                   float a, double b, msl_thing *h) MSL_NOEXCEPT;\nMSL_API long long msl_g(void) MSL_NOEXCEPT;\n"
                            "MSL_API const char *msl_s(void) MSL_NOEXCEPT;")
    assert decl["msl_f"][1][0] == ("const float[16]", "pose") and decl["msl_f"][1][8] == ("msl_thing *", "h")
    assert H().ctypes_of(decl["msl_f"]) == (None, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_uint, C.c_size_t, C.c_float, C.c_double, C.c_void_p])
    assert H().ctypes_of(decl["msl_g"]) == (C.c_longlong, []) and H().ctypes_of(decl["msl_s"]) == (C.c_char_p, [])


def test_member_lists_and_extents():
    src = "#define MSL_N 3\n#define MSL_FLAG 1u\n#define MSL_NAME text\ntypedef struct msl_a { float a, b[3], c; uint8_t d[MSL_N], e; } msl_a;"
    assert H().defines(src) == {"MSL_N": 3, "MSL_FLAG": 1}
    d = H().records(src)["msl_a"]
    assert d.names == ("a", "b", "c", "d", "e") and d.metadata["paths"] == d.names
    assert [d.fields[n][1] for n in d.names] == [0, 4, 16, 20, 23] and d.itemsize == 24
    assert d.fields["b"][0].shape == (3,) and d.fields["d"][0].shape == (3,) and d.fields["d"][0].base == "u1"


def test_nested_record_gets_c_alignment_and_padding():
    """Flattening the member list first and aligning afterwards would put s.a at 12 and t at 28, u.q's successor at 12."""
    r = H().records("typedef struct msl_in { float a; double b; } msl_in;\n"
                    "typedef struct msl_out { double d; float f; msl_in s; float t; } msl_out;\n"
                    "typedef struct msl_tail { double p; float q; } msl_tail;\n"
                    "typedef struct msl_after { msl_tail u; float v; } msl_after;")
    d = r["msl_out"]
    assert d.names == ("d", "f", "a", "b", "t") and d.metadata["paths"] == ("d", "f", "s.a", "s.b", "t")
    assert [d.fields[n][1] for n in d.names] == [0, 8, 16, 24, 32] and d.itemsize == 40
    d = r["msl_after"]
    assert [d.fields[n][1] for n in d.names] == [0, 8, 16] and d.itemsize == 24 and d.metadata["paths"] == ("u.p", "u.q", "v")
