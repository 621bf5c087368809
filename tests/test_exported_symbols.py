"""The exported surface of the engine stays what tests/golden/exported_symbols.json records: moving an entry point from one
translation unit to another must neither lose it nor leave it out of one of the two libraries
(tools/record_exported_symbols.py writes the file: the surface changes on purpose only, by recording again).  No GPU is
needed."""
import json

import exported_symbols as E


def test_both_libraries_export_the_recorded_entry_points():
    with open(E.GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(E.LIBS)
    got = {lib: E.exported(lib) for lib in E.LIBS}
    for lib in E.LIBS:
        missing, extra = sorted(set(want[lib]) - set(got[lib])), sorted(set(got[lib]) - set(want[lib]))
        assert not missing and not extra, (lib, "missing", missing, "not recorded", extra)
        assert got[lib] == want[lib], lib
    # the test-hooks library is the product with hooks compiled in: the same entry points
    product, hooks = (got[lib] for lib in E.LIBS)
    assert product == hooks, sorted(set(product) ^ set(hooks))
    print(f"{len(product)} entry points in each of {len(E.LIBS)} libraries")
    assert len(product) > 50        # (the listing itself works: the engine has far more entry points than that)
