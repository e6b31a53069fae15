"""The Python bindings above the C ABI: the signature table covers what include/oaxaca_boot.h declares, one
argument type per parameter, and each context policy of ``api.OaxacaBuilder`` raises what it raised before the
bindings shared one call scaffold. Host only."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_prototypes():
    """{name: number of parameters} of every function include/oaxaca_boot.h declares; ``(void)`` counts as 0."""
    text = open(os.path.join(ROOT, "include", "oaxaca_boot.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for name, params in re.findall(r"\b(ob_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_signature_table_and_export_list_agree(N):
    assert set(N._SIGS) == set(N.EXPORTED)
    assert len(N.EXPORTED) == len(set(N.EXPORTED))


def test_signature_table_has_one_type_per_header_parameter(N):
    protos = _header_prototypes()
    assert set(protos) == set(N._SIGS)
    wrong = {name: (len(args), protos[name]) for name, (_, args) in N._SIGS.items() if len(args) != protos[name]}
    assert not wrong, wrong


FRAME = {"wage": [10.0, 12.0, 9.0, 14.0, 11.0, 13.0, 8.0, 15.0],
         "g": ["a", "b", "a", "b", "a", "b", "a", "b"],
         "x": [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0],
         "firm": [1, 1, 2, 2, 3, 3, 4, 4]}


@pytest.fixture
def no_gpu(N):
    if N.device_count() > 0:
        pytest.skip("a GPU is visible")


def _builder(ob, predictors):
    return ob.OaxacaBuilder(FRAME, "wage", "g", "b").predictors(predictors).bootstrap_reps(4).seed(1)


def test_python_checks_come_before_the_call(ob, N, no_gpu):
    with pytest.raises(ValueError, match="unknown binary model 'nope'"):
        _builder(ob, ["x"]).prepare_binary("nope")
    with pytest.raises(N.OaxacaError) as e:
        _builder(ob, ["x"]).cluster("firm").prepare_reweighted()
    assert e.value.code == N.OB_E_UNSUPPORTED
    assert str(e.value) == "reweighted decomposition: the cluster bootstrap is outside its scope"


def test_arguments_first_reports_the_column_before_the_device(ob, N, no_gpu):
    with pytest.raises(N.OaxacaError) as e:
        _builder(ob, ["nope"]).decompose_statistics(["variance"])
    assert e.value.code == N.OB_E_COLUMN and "Column not found: nope" in str(e.value)
    with pytest.raises(N.OaxacaError) as e:
        _builder(ob, ["nope"]).optimize()
    assert e.value.code == N.OB_E_COLUMN and str(e.value) == "Column 'nope' not found in dataset."
    with pytest.raises(N.OaxacaError) as e:  # honours an explicit context, else arguments-first
        _builder(ob, ["nope"]).prepare_binary()
    assert e.value.code == N.OB_E_COLUMN and "Column not found: nope" in str(e.value)
    with pytest.raises(N.OaxacaError) as e:  # good arguments leave the missing device as the error
        _builder(ob, ["x"]).decompose_statistics(["variance"])
    assert e.value.code == N.OB_E_HIP and "no HIP device" in str(e.value)


def test_context_first_reports_the_device_before_the_column(ob, N, no_gpu):
    for call in (lambda b: b.run(), lambda b: b.prepare(), lambda b: b.efficient_frontier(2)):
        with pytest.raises(N.OaxacaError) as e:
            call(_builder(ob, ["nope"]))
        assert e.value.code == N.OB_E_HIP and "no HIP device" in str(e.value)
    with pytest.raises(N.OaxacaError) as e:
        ob.calculate_vif(FRAME, ["nope", "x"])
    assert e.value.code == N.OB_E_HIP and "no HIP device" in str(e.value)
