"""The grid of a missing-call gather that runs on the side stream beside an int8 GEMM (csrc/missing_kernels.hip: gather_blocks_beside,
sparse_rows_sum_grid), through the host-only hook fpca_debug_gather_blocks.  No device involved.

The rule: a CU has 4 SIMDs of 8 wave slots and 512 registers per lane, allocated in eights, and 160 KiB of LDS.  A GEMM workgroup of W waves puts
ceil(W / 4) waves on every SIMD; as many workgroups share a CU as slots, registers and LDS admit (at least one).  A gather block is four
waves, one per SIMD, and asks for no LDS: the blocks that stay resident beside the GEMM are what the SIMD's free slots and free registers
admit, and the limit is that times the CUs -- one block per CU where nothing is free, never zero.  Restated here in Python and compared
over the three footprints the operator meets and a grid of others; the registers of the real kernels come from the code object at run
time, the figures below are those of one build (profiles/gather_resident_ab.txt)."""
import pytest


def _alloc(r):
    return (r + 7) // 8 * 8


def _capacity(waves, vgprs, lds, gather_vgprs):
    """(GEMM workgroups sharing a CU, gather blocks resident beside them)"""
    wps = (waves + 3) // 4
    wgs = max(1, min(8 // wps, 512 // (_alloc(vgprs) * wps), (160 * 1024) // lds if lds else 8))
    return wgs, min(8 - wgs * wps, (512 - wgs * wps * _alloc(vgprs)) // _alloc(gather_vgprs))


# (waves, registers per lane, LDS bytes) of a GEMM workgroup; gather registers; workgroups per CU and blocks per CU expected
FOOTPRINTS = [
    ("exact passes: 3.5 tiles, 8 waves, one workgroup per CU", (8, 206, 133 * 1024), 48, 1, 2),
    ("exact passes, the plain gather kernel", (8, 206, 133 * 1024), 41, 1, 2),
    ("4-slice passes: 2 tiles, 4 waves, two workgroups per CU", (4, 128, 56 * 1024), 48, 2, 5),
    ("hybrid route, 256-row tiles: 3.5 tiles, 4 waves", (4, 206, 72 * 1024), 48, 2, 2),
]


@pytest.mark.parametrize("name,gemm,gather_vgprs,wgs,per_cu", FOOTPRINTS, ids=[f[0].split(":")[0] for f in FOOTPRINTS])
def test_footprints_of_the_operator(built_lib, name, gemm, gather_vgprs, wgs, per_cu):
    import flashpca_amd as fp

    assert _capacity(*gemm, gather_vgprs) == (wgs, per_cu), name
    for ncu in (256, 304, 8):
        limit, side, inline = fp.api.debug_gather_blocks(*gemm, gather_vgprs, ncu, rows_out=500224)
        assert limit == per_cu * ncu, (name, ncu)
        assert inline == 65536  # today's grid: four rows a block, at most 65536 blocks
        assert side == min(inline, limit)
    # co-resident indeed: the GEMM workgroups and the gather blocks fit the slots and the registers of a SIMD together
    wps = (gemm[0] + 3) // 4
    assert wgs * wps + per_cu <= 8 and wgs * wps * _alloc(gemm[1]) + per_cu * _alloc(gather_vgprs) <= 512


def test_rule_over_a_grid_of_footprints(built_lib):
    import flashpca_amd as fp

    seen_floor = seen_room = 0
    for waves in (1, 4, 8, 16):
        for vgprs in (24, 64, 65, 128, 129, 206, 208, 209, 256, 257, 512):
            for lds in (0, 16 * 1024, 56 * 1024, 80 * 1024, 133 * 1024, 160 * 1024):
                for gv in (8, 41, 48, 49, 64, 96, 128, 512):
                    for ncu in (1, 64, 256):
                        limit, side, inline = fp.api.debug_gather_blocks(waves, vgprs, lds, gv, ncu, rows_out=100096)
                        wgs, cap = _capacity(waves, vgprs, lds, gv)
                        assert limit >= ncu and limit % ncu == 0, "never zero: at least a block per CU"
                        assert limit // ncu == max(cap, 1), (waves, vgprs, lds, gv, ncu, limit, cap)
                        assert limit // ncu <= max(cap, 1), "never more than what is resident beside the GEMM"
                        assert inline == 100096 // 4 and side == min(inline, limit)
                        seen_floor += cap <= 0
                        seen_room += cap > 1
    assert seen_floor and seen_room


def test_inline_launches_keep_their_grid(built_lib):
    """An inline gather has the chip to itself: (rows + 3) / 4 blocks up to 65536, whatever the GEMM; a side-stream grid is never larger."""
    import flashpca_amd as fp

    for rows in (1, 3, 4, 5, 7, 1031, 2048, 2049, 4 * 65536 - 1, 4 * 65536, 4 * 65536 + 1, 1 << 31):
        limit, side, inline = fp.api.debug_gather_blocks(8, 206, 133 * 1024, 48, 256, rows_out=rows)
        assert inline == min(65536, (rows + 3) // 4)
        assert 1 <= side == min(inline, limit) and limit == 512


def test_arguments_are_checked(built_lib):
    import ctypes as C

    import flashpca_amd as fp

    L = fp.lib()
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    ok = (8, 206, 133 * 1024, 48, 256, 1000)
    assert L.fpca_debug_gather_blocks(*ok, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert L.fpca_debug_gather_blocks(*ok, None, C.byref(b), C.byref(c)) == -1 and "NULL" in L.fpca_last_error().decode()
    for i, bad in ((0, 0), (0, 17), (1, 0), (1, 513), (2, -1), (2, 160 * 1024 + 1), (3, 0), (3, 513), (4, 0), (5, 0)):
        args = list(ok)
        args[i] = bad
        assert L.fpca_debug_gather_blocks(*args, C.byref(a), C.byref(b), C.byref(c)) == -1, (i, bad)
