"""The rule that turns include/echoseal_hip.h into the ctypes binding (_native.bind_header), without a GPU: every C type spelling the
header uses against a written-out argtypes list, what the rule refuses, and the header's own vocabulary -- a new spelling fails here,
not at a call.  Last, the one kernel whose arguments DESIGN 4.22 changed keeps its resources."""
from ctypes import c_char_p, c_double, c_int, c_int64, c_uint32, c_void_p

import pytest

import echoseal_amd._native as nat

# every parameter type of the header today; the scalars are the rule's four, the rest are pointers
SCALARS = {"int", "int64_t", "uint32_t", "double"}
POINTERS = {"es_ctx*", "const es_ctx*", "void*", "const void*", "const char*", "uint8_t*", "const uint8_t*", "int8_t*", "int32_t*",
            "const int32_t*", "uint32_t*", "const uint32_t*", "int64_t*", "const int64_t*", "uint64_t*", "const uint64_t*", "float*",
            "const float*", "double*", "const double*"}

SYNTHETIC = """
/* a comment with a declaration in it: int es_not_this(int a); */
#define ES_TEN        10     /* decimal */
#define ES_HEX      0x1Fu
#define ES_NEG      (-3)
#define ES_SHIFT    (1 << 20)
#define ES_WIDE     0xFFFFFFFFFFFFFFFFull
#define NOT_OURS    (sizeof(int))
typedef struct es_ctx es_ctx;
es_ctx*     es_make(int device, int n);
void        es_drop(es_ctx* ctx);
const char* es_text(const es_ctx* ctx);
int         es_version(void);
int es_scalars(es_ctx* ctx, int a, int64_t b, uint32_t c, double d);
int es_bytes(es_ctx* ctx, const uint8_t* key32_host, const uint8_t* key_dev, const char* name, uint8_t* out_host,
             const int64_t* rec_host);
int es_pointers_batch(es_ctx* ctx, const void* x_dev, const double* y_dev /* nullable */, float *spaced_dev, const float * both_dev,
                      int8_t* ok_dev, const int32_t* i_dev, int32_t* j_dev, const uint32_t* u_dev, uint32_t* v_dev, int64_t* n_dev,
                      const uint64_t* k_dev, uint64_t* t_dev, double* z_dev, void* stream);
"""


def test_rule_on_synthetic_declarations():
    decl, sig, const = nat.bind_header(SYNTHETIC)
    assert const == {"ES_TEN": 10, "ES_HEX": 31, "ES_NEG": -3, "ES_SHIFT": 1 << 20, "ES_WIDE": 2 ** 64 - 1}
    assert sig == {
        "es_make": (c_void_p, [c_int, c_int]),
        "es_drop": (None, [c_void_p]),
        "es_text": (c_char_p, [c_void_p]),
        "es_version": (c_int, []),
        "es_scalars": (c_int, [c_void_p, c_int, c_int64, c_uint32, c_double]),
        # bytes objects: `const char*` and a `const uint8_t*` whose name ends in _host -- nothing else, whatever its name
        "es_bytes": (c_int, [c_void_p, c_char_p, c_void_p, c_char_p, c_void_p, c_void_p]),
        "es_pointers_batch": (c_int, [c_void_p] * 15),
    }
    assert decl["es_version"] == [] and decl["es_scalars"] == [("es_ctx*", "ctx"), ("int", "a"), ("int64_t", "b"), ("uint32_t", "c"), ("double", "d")]
    assert decl["es_pointers_batch"][2:5] == [("const double*", "y_dev"), ("float*", "spaced_dev"), ("const float*", "both_dev")]
    assert decl["es_pointers_batch"][-1] == ("void*", "stream")
    used = {t for params in decl.values() for t, _ in params}
    assert used == SCALARS | POINTERS                                       # the synthetic header spells every type of the vocabulary


@pytest.mark.parametrize("text,names", [
    ("int es_f(es_ctx* ctx, size_t n);", ("es_f", "size_t n")),
    ("int es_f(es_ctx* ctx, float gain);", ("es_f", "float gain")),
    ("int es_f(es_ctx* ctx, const uint8_t** rows_dev);", ("es_f", "rows_dev")),
    ("float es_f(es_ctx* ctx);", ("es_f", "float")),
    ("#define ES_BAD (1 + 2)", ("ES_BAD", "1 + 2")),
    ("#define ES_BAD sizeof(int)", ("ES_BAD", "sizeof(int)")),
    ("#define ES_BAD 1.5", ("ES_BAD", "1.5")),
])
def test_rule_refuses_by_name(text, names):
    with pytest.raises(nat.NativeError) as e:
        nat.bind_header(text)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_the_header_stays_inside_the_vocabulary():
    used = {t for params in nat.DECLARATIONS.values() for t, _ in params}
    assert used <= SCALARS | POINTERS, used - (SCALARS | POINTERS)
    assert len(nat.DECLARATIONS) == len(nat.SIGNATURES) == 56
    for name, value in nat.CONSTANTS.items():                               # every ES_* define is a module constant of the binding
        assert getattr(nat, name) == value and isinstance(value, int), name
    assert nat.ES_ABI_VERSION == 2 and nat.ES_XC_SEG == 1216 and nat.ES_RESAMPLE_TABLE_MAX == 1 << 30 and nat.ES_EINVAL == -1
    # a 64-bit size is bound as one: an `int` in its place would pass every argument count
    for name, params in nat.DECLARATIONS.items():
        for (ctype, _), arg in zip(params, nat.SIGNATURES[name][1]):
            assert (arg is c_int64) == (ctype == "int64_t") and (arg is c_int) == (ctype == "int"), (name, ctype)


def test_the_header_pn_by_value_costs_the_symbol_kernel_nothing(tmp_path):
    """es_tx_symbols_kernel takes its 16 header-PN bytes as a struct argument: still no private segment, no flat or scratch
    access, and the VGPR count written down there."""
    from code_objects import code_objects, disassembly, kernel_metadata
    md, funcs = {}, {}
    for co in code_objects(tmp_path):
        md.update(kernel_metadata(co))
        funcs.update(disassembly(co))
    hits = [k for k in md if "es_tx_symbols_kernel" in k]
    assert len(hits) == 1 and "HdrPn" in hits[0], hits
    m = md[hits[0]]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["vgpr_count"] == 22, m
    assert funcs[hits[0]] and not [i for i in funcs[hits[0]] if i.startswith(("flat_", "scratch_"))]
