from echoseal_amd.issuer import *  # noqa: F401,F403  (the many-key embedder, under the reference's package name)
from echoseal_amd import issuer as _impl
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith('__')})
