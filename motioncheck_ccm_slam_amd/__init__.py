"""MI355X hot path of CCM-SLAM.  The submodules are imported on demand; the map-point table and the TrackLocalMap calls on it are
also reachable from the package itself."""


def __getattr__(name):
    if name in ("MapPointTable", "Tracking"):
        from . import tracking
        return getattr(tracking, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
