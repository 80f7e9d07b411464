"""The cases of spmv_stream_cases.py have the slices they are there for (the builders assert it against the restated layout
of csrc/panel.hip), and their exact products exist in both variants.  No GPU."""
import numpy as np
import pytest

import spmv_cases as sc
import spmv_stream_cases as ssc


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("name", ["ladder", "lone_row", "last_local_row"])
def test_builders(name, variant):
    case = getattr(ssc, name)(variant)
    prods = case.products()
    assert (prods[0].exact_int is not None) == (variant == "int")
    assert all(np.all(np.isfinite(p.exact)) for p in prods.values())


def test_ladder_covers_every_shortfall():
    short = [ssc.LADDER[0] - k for k in ssc.LADDER]
    assert sorted(set(short)) == list(range(40)) and ssc.LADDER[0] == 40 and ssc.LADDER == sorted(ssc.LADDER, reverse=True)


def test_a_full_tile_fits_the_table():
    assert ssc.TILE_ROWS - 1 == 0x0F7F < 0xFFFF
    # the cost floor of a (group, row) cell makes a tile exactly 3968 rows with one and with two panels per group
    for group in ssc.GROUPS:
        budget = ssc.LAST_ROW_TILE_NNZ * group
        cmin = -(-budget // ssc.TILE_ROWS)
        assert cmin >= 17 and budget == cmin * ssc.TILE_ROWS
