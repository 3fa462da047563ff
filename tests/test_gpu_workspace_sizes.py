"""The *_workspace_bytes functions against a literal table.

Callers allocate by these functions and the kernels index the carved members,
so no workspace may grow, shrink or move when the host code that carves them
is rewritten.  The numbers are the `total` columns of
profiles/capi_ws/layout_parent.txt: the output of tools/dbg/ws_layout_dump.cpp
built on the tree from before the carving went through one helper -- never
the output of the code under test.  Needs a context (hence a device) but
launches nothing.

The shapes are the smallest that reach every branch of the carving: N below
one block, N no multiple of 64, each tier of the automatic outer panel width
(256 below N = 2048, 384 up to 4096, 512 above), and after set_blocking
nbi = 128 (no persistent-solve prep region) and an explicit nbo.
"""
import pytest

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")

NRHS = (2, 8, 257)
# (nbo, nbi) given to set_blocking ((0, 64): the default) -> N -> (ldlt, mixed, mixed_multi per NRHS)
TABLE = {
    (0, 64): {
        1: (669696, 387584, (1792, 3328, 80384)),
        65: (1095680, 638208, (3328, 9472, 281856)),
        320: (3818752, 2401280, (8704, 32256, 1013504)),
        2047: (22190848, 28558848, (50944, 201472, 6453504)),
        2560: (35581440, 45022976, (63488, 251648, 8065536)),
        4097: (70023168, 105604096, (102144, 404736, 12975616)),
    },
    (128, 128): {
        65: (438272, 538368, (3328, 9472, 281856)),
        2560: (10695424, 37175296, (63488, 251648, 8065536)),
    },
    (512, 64): {
        65: (1495040, 837888, (3328, 9472, 281856)),
        2560: (43443200, 48952576, (63488, 251648, 8065536)),
    },
}
# the normal-equations workspace at the default blocking: the file's three (n, mp) lines
NORMAL = {(64, 0): 1057024, (100, 37): 2099456, (2048, 512): 35581696}
CASES = [(b, N) for b, rows in TABLE.items() for N in rows]


@pytest.fixture(scope="module")
def ctx():
    c = I.Context(0)
    yield c
    c.set_blocking(0, 64)


@pytest.mark.parametrize("blocking,N", CASES, ids=[f"nbo{b[0]}-nbi{b[1]}-N{N}" for b, N in CASES])
def test_workspace_bytes(ctx, blocking, N):
    ldlt, mixed, multi = TABLE[blocking][N]
    ctx.set_blocking(*blocking)
    try:
        got = (ctx.workspace_bytes(N), ctx.mixed_workspace_bytes(N),
               tuple(ctx.mixed_multi_workspace_bytes(N, r) for r in NRHS))
        # the layout file's normal lines are 256 bytes (the definiteness info word) + the order n + mp
        # LDL^T workspace: the same relation for this order, split as n = N - N // 4, mp = N // 4
        normal = ctx.normal_workspace_bytes(N - N // 4, N // 4)
    finally:
        ctx.set_blocking(0, 64)
    print(f"blocking={blocking} N={N}: ldlt {got[0]} mixed {got[1]} mixed_multi {got[2]} normal {normal}")
    assert got == (ldlt, mixed, multi)
    assert normal == 256 + ldlt


@pytest.mark.parametrize("n,mp", list(NORMAL))
def test_normal_workspace_bytes(ctx, n, mp):
    got = ctx.normal_workspace_bytes(n, mp)
    print(f"normal n={n} mp={mp}: {got}")
    assert got == NORMAL[(n, mp)]
