"""ppsci.data.transform (/root/reference/ppsci/data/process/transform/__init__.py:42-72, preprocess.py:287-331): the
`transforms` of a dataset config -- a list of {ClassName: kwargs} -- as one callable on (input, label, weight).

Only FunctionalTransform is built (the fPINN example grows its batch with it, examples/fpde/fractional_poisson_2d.py:86-130);
any other name raises instead of being dropped."""
from __future__ import annotations

from typing import Callable, Dict, Tuple

import numpy as np

__all__ = ["Compose", "FunctionalTransform", "build_transforms"]


class Compose:
    """Applies the transforms in order, each to the whole (input, label, weight) tuple the previous one returned."""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, *data):
        for f in self.transforms:
            data = f(*data)
        return data


class FunctionalTransform:
    """transform_func(input, label, weight) on shallow copies of the three dicts (weight None -> {})."""

    def __init__(self, transform_func: Callable):
        self.transform_func = transform_func

    def __call__(self, *data: Dict[str, np.ndarray]) -> Tuple[Dict[str, np.ndarray], ...]:
        data_dict, label_dict, weight_dict = data
        return self.transform_func({**data_dict}, {**label_dict}, {**weight_dict} if weight_dict is not None else {})


def build_transforms(cfg):
    """A callable passes through unchanged; a config list becomes a Compose; an unknown name raises NotImplementedError."""
    if cfg is None or callable(cfg):
        return cfg
    if not cfg:
        return Compose([])
    ts = []
    for item in cfg:
        name = next(iter(item.keys()))
        if name != "FunctionalTransform":
            raise NotImplementedError(f"dataset transform {name!r}: only FunctionalTransform is built")
        ts.append(FunctionalTransform(**dict(item[name])))
    return Compose(ts)
