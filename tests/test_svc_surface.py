"""CPU: plssvm_amd.svc.SVC as a scikit-learn estimator -- the reference's keywords and parameters (bindings/Python/sklearn.cpp), get_params / set_params in
scikit-learn's contract, and the fitted attributes, absent before fit."""

import numpy as np
import pytest

from plssvm_amd import csvm
from plssvm_amd.svc import SVC

FITTED = ["classes_", "fit_status_", "n_features_in_", "shape_fit_", "n_iter_", "class_weight_", "support_", "support_vectors_", "n_support_", "dual_coef_",
          "intercept_", "coef_"]
NOT_IMPLEMENTED = ["shrinking", "probability", "cache_size", "decision_function_shape", "break_ties", "random_state"]


def test_get_params_set_params_and_clone():
    sklearn_base = pytest.importorskip("sklearn.base")
    est = SVC(C=3, kernel="linear", class_weight="balanced")
    params = est.get_params()
    assert sorted(params) == sorted(["C", "kernel", "degree", "gamma", "coef0", "tol", "verbose", "max_iter", "class_weight", "real_type"])
    assert params["C"] == 3 and params["kernel"] == "linear" and params["class_weight"] == "balanced" and params["real_type"] is np.float64
    assert est.get_params(deep=False) == params
    twin = sklearn_base.clone(est)
    assert twin is not est and twin.get_params() == params
    cw = {1: 2.0, -1: 0.5}
    twin = sklearn_base.clone(SVC(class_weight=cw, gamma=0.25, real_type=np.float32))
    assert twin.class_weight == cw and twin.gamma == 0.25 and twin.real_type is np.float32
    assert est.set_params(C=2) is est and est.C == 2 and est.get_params()["C"] == 2
    assert est.set_params(kernel="rbf", tol=1e-6, max_iter=10) is est and (est.kernel, est.tol, est.max_iter) == ("rbf", 1e-6, 10)
    with pytest.raises(ValueError, match="no_such_parameter"):
        est.set_params(no_such_parameter=1)
    with pytest.raises(TypeError):
        SVC(no_such_parameter=1)


@pytest.mark.parametrize("name", NOT_IMPLEMENTED)
def test_keywords_the_reference_rejects(name):
    text = f"The '{name}' parameter for a call to the 'SVC' constructor is not implemented yet!"
    with pytest.raises(AttributeError) as e:
        SVC(**{name: True})
    assert str(e.value) == text
    with pytest.raises(AttributeError) as e:
        SVC().set_params(**{name: True})
    assert str(e.value) == text


def test_verbose_sets_the_library_verbosity():
    before = csvm.verbosity
    try:
        SVC(verbose=True)
        assert csvm.verbosity == "full"
        SVC().set_params(verbose=False)
        assert csvm.verbosity == "quiet"
    finally:
        csvm.verbosity = before


def test_fitted_attributes_are_absent_before_fit():
    est = SVC()
    for name in FITTED:
        assert not hasattr(est, name), name
        with pytest.raises(AttributeError) as e:
            getattr(est, name)
        assert str(e.value) == f"'SVC' object has no attribute '{name}'"
    for name in ("probA_", "probB_", "feature_names_in_"):
        with pytest.raises(AttributeError) as e:
            getattr(est, name)
        assert str(e.value) == f"'SVC' object has no attribute '{name}' (not implemented)"
    for name in ("predict_proba", "predict_log_proba"):
        assert not hasattr(est, name)
        with pytest.raises(AttributeError) as e:
            getattr(est, name)
        assert str(e.value) == f"'SVC' object has no function '{name}' (not implemented)"
    with pytest.raises(AttributeError, match="not fitted yet"):
        est.decision_function(np.ones((2, 3)))
    validation = pytest.importorskip("sklearn.utils.validation")
    exceptions = pytest.importorskip("sklearn.exceptions")
    with pytest.raises(exceptions.NotFittedError):
        validation.check_is_fitted(est)
