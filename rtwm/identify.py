from echoseal_amd.identify import *  # noqa: F401,F403  (the many-key detector, under the reference's package name)
from echoseal_amd import identify as _impl
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith('__')})
