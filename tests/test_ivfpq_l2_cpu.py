"""The L2 search's per-key term at the C-ABI boundary (include/gnnlm.h, ABI 12 additive entries): the new entry point is
declared and exported, `key_term` is the scan descriptor's LAST member (nothing before it moved), and the generated ctypes
mirror has the size the C compiler sees.  No compute calls."""
import ctypes

from gnnlm_amd import _lib


def test_key_terms_entry_is_declared_and_exported():
    assert "gnnlm_ivfpq_key_terms" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "gnnlm_ivfpq_key_terms")


def test_scan_descriptor_ends_with_key_term():
    st = _lib.gnnlm_ivfpq_scan_t
    names = [f[0] for f in st._fields_]
    assert names[-1] == "key_term" and st._fields_[-1][1] is ctypes.c_void_p
    assert names[-3:-1] == ["list_term", "ld_list_term"]                    # appended: the members before it keep their places
    assert names[0] == "codes" and names.index("packed") < names.index("list_term")
    assert _lib.lib().gnnlm_sizeof(b"gnnlm_ivfpq_scan_t") == ctypes.sizeof(st)
    assert st.key_term.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(st)
    assert _lib.ABI_VERSION == 12
