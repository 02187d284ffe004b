"""ConfigSpace binding: the real package when installed, else the engine's compatible stand-in."""
try:  # pragma: no cover - depends on the environment
    import ConfigSpace  # noqa: F401
    import ConfigSpace.util  # noqa: F401  (deactivate_inactive_hyperparameters, for conditional spaces)
except ImportError:  # ConfigSpace is not part of this image
    from .. import configspace as ConfigSpace  # noqa: F401
