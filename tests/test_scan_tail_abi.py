"""The scan merge's C ABI (csrc/scan_tail.hip, csrc/scan_merge_check.cpp), no GPU needed: include/radnet_hip.h, radnet_hip.lib's
mirror structs and signatures and the symbols libradnet_hip.so exports agree, the constants the kernels, the bindings and the tests
share are the header's, and the host-only entries (the size queries, radnet_scan_merge_check) answer without a device."""
import ctypes as C
import os
import re

import numpy as np

from radnet_hip import lib as L

CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double, "float": C.c_float, "int": C.c_int}
STRUCTS = {"radnet_final_nms_desc": "FinalNmsDesc", "radnet_scan_tile": "ScanTile", "radnet_scan_merge_desc": "ScanMergeDesc"}
ENTRIES = ("radnet_final_nms_ws_bytes", "radnet_final_nms", "radnet_scan_merge_out_bytes", "radnet_scan_merge_ws_bytes", "radnet_scan_merge",
           "radnet_scan_merge_check")


def header():
    return re.sub(r"/\*.*?\*/", "", open(L.HEADER_PATH).read(), flags=re.S)


def ctype_of(decl):
    """The ctypes type of a C declaration's type part: every pointer travels as void* (char* as c_char_p, int32_t* as a pointer)."""
    decl = decl.replace("const ", "").strip()
    if decl.endswith("*"):
        base = decl[:-1].strip()
        if base == "char":
            return C.c_char_p
        if base == "int32_t":
            return C.POINTER(C.c_int32)
        return C.c_void_p
    return CTYPE[decl]


def struct_fields(name):
    m = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (name, name), header(), flags=re.S)
    assert m is not None, name
    fields = []
    for stmt in m.group(1).split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        first, *more = [p.strip() for p in stmt.split(",")]
        words = first.replace("*", "* ").split()
        kind = " ".join(words[:-1]).replace(" *", "*")
        for field in [words[-1]] + more:
            fields.append((field, ctype_of(kind)))
    return fields


def test_structs_mirror_the_header():
    for cname, pyname in STRUCTS.items():
        want = struct_fields(cname)
        got = [(n, t) for n, t in getattr(L, pyname)._fields_]
        assert [n for n, _ in got] == [n for n, _ in want], cname
        for (n, t), (_, w) in zip(got, want):
            assert C.sizeof(t) == C.sizeof(w) and (t is w or w is C.c_void_p or t is C.c_void_p), (cname, n, t, w)
    assert C.sizeof(L.ScanTile) == 16
    from radnet_hip.engine import SCAN_TILE
    assert SCAN_TILE.itemsize == 16 and list(SCAN_TILE.names) == [n for n, _ in L.ScanTile._fields_]
    d = L.FinalNmsDesc
    assert (d.n_groups.offset, d.obj_avg_threshold.offset, d.obj_confidence_threshold.offset, d.n_obj_avg.offset, d.out_boxes.offset, d.ws.offset) \
        == (24, 32, 40, 44, 48, 80) and C.sizeof(d) == 88
    m = L.ScanMergeDesc
    assert (m.pool_words.offset, m.slot_rows.offset, m.tiles_host.offset, m.n_tiles.offset, m.obj_avg_threshold.offset, m.n_obj_avg.offset,
            m.nms_thresh.offset, m.max_boxes.offset, m.out.offset, m.ws.offset) == (8, 16, 24, 40, 48, 60, 64, 72, 80, 88) and C.sizeof(m) == 96


def prototype(name):
    m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m is not None, name
    args = []
    for p in m.group(2).split(","):
        words = p.replace("*", "* ").split()
        args.append(" ".join(words[:-1]).replace(" *", "*"))
    return m.group(1), args


def _lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def test_signatures_match_the_header_and_the_library():
    declared = L.declared_symbols()
    lib = _lib()
    for name in ENTRIES:
        assert name in declared, name
        res, args = prototype(name)
        fn = getattr(lib, name)                          # exported
        assert fn.restype is CTYPE[res], name
        assert len(fn.argtypes) == len(args), name
        for got, decl in zip(fn.argtypes, args):
            base = decl.replace("const ", "").rstrip("*").strip()
            if base in STRUCTS:
                assert got is C.POINTER(getattr(L, STRUCTS[base])) or got is C.c_void_p, (name, decl)
            elif decl.endswith("*"):
                assert got in (C.c_void_p, C.c_char_p) or got is C.POINTER(C.c_int32), (name, decl)
            else:
                assert got is CTYPE[decl], (name, decl, got)


def test_constants_are_the_header_s():
    import scan_tail_cases as S
    assert L.header_constant("RADNET_SCAN_MAX_COORD") == S.MAX_COORD == 1 << 29
    assert [L.header_constant("RADNET_FINAL_NMS_" + k) for k in ("MALFORMED", "EMPTY", "RANGE")] == [S.FN_MALFORMED, S.FN_EMPTY, S.FN_RANGE]
    assert [L.header_constant("RADNET_SCAN_MERGE_" + k) for k in ("BAD_SLOT", "MALFORMED", "EMPTY", "RANGE", "NMS_BOX")] \
        == [S.SM_BAD_SLOT, S.SM_MALFORMED, S.SM_EMPTY, S.SM_RANGE, S.SM_NMS_BOX]
    assert (L.DETECT_HEADER, L.DETECT_RECORD) == (S.HEADER, S.RECORD)
    assert L.header_constant("RADNET_SCAN_MAX_CLASSES") == 32


def test_host_only_entries_answer_without_a_device():
    import scan_tail_cases as S
    lib = _lib()
    assert lib.radnet_scan_merge_out_bytes(7, 300) == 4 * S.scan_merge_out_words(7, 300)
    assert lib.radnet_scan_merge_out_bytes(-1, 300) == 0
    assert lib.radnet_final_nms_ws_bytes(0, 0) > 0 and lib.radnet_final_nms_ws_bytes(-1, 0) == 0
    small, large = lib.radnet_final_nms_ws_bytes(1000, 4), lib.radnet_final_nms_ws_bytes(2000, 4)
    assert 48 * 1000 <= small < large <= 2 * small + 4096                      # grows with the capacity, and with nothing else
    assert lib.radnet_scan_merge_ws_bytes(37, 300, 1, 7, 300) > lib.radnet_final_nms_ws_bytes(37 * 300, 7)
    assert lib.radnet_scan_merge_ws_bytes(-1, 300, 1, 7, 300) == 0
    sw = S.slot_words(300)
    table = np.array([(0, 0, 0, 0), (sw, 250, 0, 0), (2 * sw, 0, 0, 1)], np.int32)
    assert L.scan_merge_check(table, 3 * sw, 300) == (0, 2, -2, "")
    rc, n_images, bad, msg = L.scan_merge_check(table, 3 * sw - 1, 300)
    assert rc != 0 and n_images == 0 and bad == 2 and "slot" in msg
    table[2, 0] = sw + 2
    rc, n_images, bad, msg = L.scan_merge_check(table, 3 * sw, 300)
    assert rc != 0 and bad == 2 and "overlaps" in msg
    assert L.scan_merge_check(None, 0, 300)[:2] == (0, 0)
    assert L.scan_merge_check(None, 0, 300, count=5)[0] != 0                   # a null table of five tiles
