"""FA_VARIANT_AUTO's routing, pinned: fa_resolve_variant_for and fa_fwd_kernel_name over a grid of dtypes, head dims, sequence
lengths (every threshold of the rule and its neighbours), head counts and both masks, against tests/golden/auto_routes.json, which
was recorded from the library as it stood before the host layer was refactored. CPU only: nothing here launches.

Regenerate (only when a change to the rule is intended): python tests/test_auto_routes.py"""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "auto_routes.json")

DTYPES = (0, 1, 2, 3)  # f32, f16, bf16, e4m3
HEAD_DIMS = tuple(range(8, 257, 8)) + (4, 44, 60, 100, 130)
SEQLENS = (64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 4095, 4096,
           4097, 8191, 8192, 8193, 16384)
HEADS = ((1, 8), (2, 8), (4, 8), (6, 8), (8, 8), (4, 24), (16, 8), (8, 32), (16, 32), (64, 8), (32, 32), (64, 32))  # (B, H): 8 .. 2048


def _rle(tokens):
    out, prev, n = [], None, 0
    for t in tokens + [None]:
        if t == prev:
            n += 1
            continue
        if prev is not None:
            out.append(f"{prev}*{n}" if n > 1 else str(prev))
        prev, n = t, 1
    return " ".join(out)


def routes(lib):
    """{"routes": [distinct "variant|kernel name"], "rows": {"dtype/D/causal": run-length encoded route indices over (B, H) x N}}"""
    names, rows = {}, {}
    for dtype in DTYPES:
        for D in HEAD_DIMS:
            for causal in (0, 1):
                toks = []
                for B, H in HEADS:
                    for N in SEQLENS:
                        v = lib.fa_resolve_variant_for(dtype, D, B, H, N, causal)
                        key = f"{lib.fa_variant_name(v).decode() if v >= 0 else v}|{lib.fa_fwd_kernel_name(dtype, D, B, H, N, causal).decode()}"
                        toks.append(names.setdefault(key, len(names)))
                rows[f"{dtype}/{D}/{causal}"] = _rle(toks)
    return {"grid": {"dtypes": DTYPES, "head_dims": HEAD_DIMS, "seqlens": SEQLENS, "heads": HEADS},
            "routes": sorted(names, key=names.get), "rows": rows}


def _decode(table):
    """the fixture as {(dtype, D, causal, B, H, N): "variant|kernel name"}"""
    g, out = table["grid"], {}
    for key, row in table["rows"].items():
        dtype, D, causal = map(int, key.split("/"))
        toks = [int(t) for tok in row.split() for t in [tok.split("*")[0]] * (int(tok.split("*")[1]) if "*" in tok else 1)]
        pts = [(B, H, N) for B, H in g["heads"] for N in g["seqlens"]]
        assert len(toks) == len(pts), key
        for (B, H, N), t in zip(pts, toks):
            out[(dtype, D, causal, B, H, N)] = table["routes"][t]
    return out


def test_auto_routes_match_the_recorded_table():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    with open(FIXTURE) as f:
        want = json.load(f)
    got = routes(fa.load_library())
    assert json.loads(json.dumps(got["grid"])) == want["grid"]
    expect, have = _decode(want), _decode(json.loads(json.dumps(got)))
    assert len(expect) == len(DTYPES) * len(HEAD_DIMS) * 2 * len(HEADS) * len(SEQLENS)
    diff = [(k, expect[k], have[k]) for k in expect if expect[k] != have[k]]
    assert not diff, diff[:20]
    # the grid reaches every kernel AUTO can pick
    assert {r.split("|")[0] for r in want["routes"]} == {"mfma", "mfma16", "mfma_splitkv", "mfma_split2", "mfma_h64s2", "mfma_fp8pv",
                                                        "tiled_v2", "-2"}


if __name__ == "__main__":
    import sys

    sys.path.insert(0, ROOT)
    import flash_attention_metal_amd as fa

    t = routes(fa.load_library())
    lines = ['{"grid": ' + json.dumps(t["grid"]) + ",", '"routes": [', ",\n".join("  " + json.dumps(r) for r in t["routes"]), "],",
             '"rows": {', ",\n".join(f"  {json.dumps(k)}: {json.dumps(r)}" for k, r in t["rows"].items()), "}}"]
    with open(FIXTURE, "w") as f:
        f.write("\n".join(lines) + "\n")
