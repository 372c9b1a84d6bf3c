"""ppsci.data.process (/root/reference/ppsci/data/process/__init__.py): the sample transforms of the datasets."""
from . import transform  # noqa: F401
