"""delta_graph_slam_amd -- MI355X-native scan registration (NDT / GICP) hot path."""

__all__ = ["MapCloudGenerator", "LineExtractor", "LineScanMatcher", "BuildingOverlap", "FloorDetector", "BuildingClouds"]


def __getattr__(name):   # resolved on first use: importing the package alone loads neither torch nor the HIP library
    if name == "MapCloudGenerator":
        from .map_cloud import MapCloudGenerator
        return MapCloudGenerator
    if name == "LineExtractor":
        from .line_extraction import LineExtractor
        return LineExtractor
    if name == "LineScanMatcher":
        from .line_align import LineScanMatcher
        return LineScanMatcher
    if name == "BuildingOverlap":
        from .building_overlap import BuildingOverlap
        return BuildingOverlap
    if name == "FloorDetector":
        from .floor_detection import FloorDetector
        return FloorDetector
    if name == "BuildingClouds":
        from .building_cloud import BuildingClouds
        return BuildingClouds
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
