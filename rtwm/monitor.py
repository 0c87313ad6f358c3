from echoseal_amd.monitor import *  # noqa: F401,F403  (the live monitor's table and layout, under the reference's package name)
from echoseal_amd import monitor as _impl
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith('__')})
