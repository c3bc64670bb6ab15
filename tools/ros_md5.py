#!/usr/bin/env python3
"""ROS-1 md5sums of the nine vision_slam_frontend messages (MESSAGES below: the field lists of the reference's msg/*.msg, the
wire contract host/slam_to_ros.h serialises), by genmsg's rule (gentools.compute_md5_text, what `rosmsg md5` / gendeps print):

    comments and blank lines dropped; constants first as "type name=value"; then one line per field, "type name" for a
    builtin type (array suffix kept) and "<md5 of the sub-message> name" for a message type (array suffix dropped);
    lines joined by '\\n', no trailing newline; md5 of that text.

A bag writer needs them for its connection headers (md5sum=, type=vision_slam_frontend/<Name>).  geometry_msgs' three
messages are restated here; their md5sums are known constants of every ROS-1 distribution and pin the rule:
Point = Vector3 = 4a842b65f413084dc2b10fb484ea7f17, Quaternion = a779879fadf0160734f906b8c19c7004.

    python tools/ros_md5.py            prints the table
    python tools/ros_md5.py --header   prints the constants of host/slam_to_ros.h"""
import hashlib
import sys

MESSAGES = {  # message -> its field list, "type name" per line (comments of the .msg files do not enter the md5sum)
    'CameraExtrinsics': 'float64[3] translation\nfloat64[3] rotation',
    'CameraIntrinsics': 'float64 fx\nfloat64 fy\nfloat64 cx\nfloat64 cy',
    'FeatureMatch': 'uint64 id_initial\nuint64 id_current',
    'OdometryFactor': 'uint64 pose_i\nuint64 pose_j\ngeometry_msgs/Vector3 translation\ngeometry_msgs/Quaternion rotation',
    'RobotPose': 'geometry_msgs/Vector3 loc\ngeometry_msgs/Quaternion angle',
    'SLAMNode': 'uint64 id\nfloat64 timestamp\nRobotPose pose\nVisionFeature[] features',
    'SLAMProblem': 'SLAMNode[] nodes\nVisionFactor[] vision_factors\nOdometryFactor[] odometry_factors',
    'VisionFactor': 'uint64 pose_initial\nuint64 pose_current\nFeatureMatch[] feature_matches',
    'VisionFeature': 'uint64 id\ngeometry_msgs/Point pixel\ngeometry_msgs/Point point3d',
}
PACKAGE = "vision_slam_frontend"
BUILTIN = {"bool", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float32", "float64", "string",
           "time", "duration", "char", "byte"}
GEOMETRY = {
    "geometry_msgs/Point": "float64 x\nfloat64 y\nfloat64 z\n",
    "geometry_msgs/Vector3": "float64 x\nfloat64 y\nfloat64 z\n",
    "geometry_msgs/Quaternion": "float64 x\nfloat64 y\nfloat64 z\nfloat64 w\n",
    "geometry_msgs/Pose": "Point position\nQuaternion orientation\n",
}
KNOWN = {"geometry_msgs/Point": "4a842b65f413084dc2b10fb484ea7f17", "geometry_msgs/Vector3": "4a842b65f413084dc2b10fb484ea7f17",
         "geometry_msgs/Quaternion": "a779879fadf0160734f906b8c19c7004",
         "std_msgs/Header": "2176decaecbce78abc3b96ef049fabed", "sensor_msgs/CompressedImage": "8f7a12909da2c9d3332d540a0977563f",
         "geometry_msgs/Pose": "e45d45a5a1ce597b249e23fb30fc871f", "std_msgs/ColorRGBA": "a29a96539573343b1310c73607334b00"}
# The one message of another package the host serialises: sensor_msgs/CompressedImage (the debug images as JPEG files), with the
# std_msgs/Header it starts with.  Field lists of ROS-1's common_msgs / std_msgs; not part of table() (the package's own nine).
EXTERNAL = {
    "std_msgs/Header": "uint32 seq\ntime stamp\nstring frame_id\n",
    "sensor_msgs/CompressedImage": "Header header\nstring format\nuint8[] data\n",
    # ... and the two the driver's PublishVisualization sends to RViz (host/slam_visualization.h, slam_to_ros.h SerializeMarker /
    # SerializeMarkerArray): visualization_msgs/Marker as ROS-1 ships it since DELETEALL was added (Jade), and MarkerArray
    "std_msgs/ColorRGBA": "float32 r\nfloat32 g\nfloat32 b\nfloat32 a\n",
    "visualization_msgs/Marker": (
        "uint8 ARROW=0\nuint8 CUBE=1\nuint8 SPHERE=2\nuint8 CYLINDER=3\nuint8 LINE_STRIP=4\nuint8 LINE_LIST=5\nuint8 CUBE_LIST=6\n"
        "uint8 SPHERE_LIST=7\nuint8 POINTS=8\nuint8 TEXT_VIEW_FACING=9\nuint8 MESH_RESOURCE=10\nuint8 TRIANGLE_LIST=11\n"
        "uint8 ADD=0\nuint8 MODIFY=0\nuint8 DELETE=2\nuint8 DELETEALL=3\n"
        "Header header\nstring ns\nint32 id\nint32 type\nint32 action\ngeometry_msgs/Pose pose\ngeometry_msgs/Vector3 scale\n"
        "std_msgs/ColorRGBA color\nduration lifetime\nbool frame_locked\ngeometry_msgs/Point[] points\n"
        "std_msgs/ColorRGBA[] colors\nstring text\nstring mesh_resource\nbool mesh_use_embedded_materials\n"),
    "visualization_msgs/MarkerArray": "Marker[] markers\n",
}
NAMES = ["CameraExtrinsics", "CameraIntrinsics", "FeatureMatch", "OdometryFactor", "RobotPose", "SLAMNode", "SLAMProblem",
         "VisionFactor", "VisionFeature"]


def msg_text(full_name: str) -> str:
    if full_name in GEOMETRY:
        return GEOMETRY[full_name]
    if full_name in EXTERNAL:
        return EXTERNAL[full_name]
    pkg, name = full_name.split("/")
    assert pkg == PACKAGE, full_name
    return MESSAGES[name] + "\n"


def md5_text(full_name: str) -> str:
    pkg = full_name.split("/")[0]
    consts, fields = [], []
    for line in msg_text(full_name).splitlines():
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        type_, rest = line.split(None, 1)
        if "=" in rest:
            name, val = rest.split("=", 1)
            consts.append("%s %s=%s" % (type_, name.strip(), val.strip()))
            continue
        name = rest.strip()
        bare = type_.split("[", 1)[0]
        if bare in BUILTIN:
            fields.append("%s %s" % (type_, name))
        else:
            sub = bare if "/" in bare else ("std_msgs/Header" if bare == "Header" else "%s/%s" % (pkg, bare))
            fields.append("%s %s" % (md5(sub), name))
    return "\n".join(consts + fields)


def md5(full_name: str) -> str:
    return hashlib.md5(md5_text(full_name).encode()).hexdigest()


def table() -> dict:
    for k, v in KNOWN.items():
        assert md5(k) == v, (k, md5(k), v)  # the rule reproduces the md5sums every ROS-1 installation carries
    return {n: md5("%s/%s" % (PACKAGE, n)) for n in NAMES}


def marker_md5s() -> tuple:
    """md5sums of visualization_msgs/Marker and MarkerArray (slam_to_ros.h: kMarkerMd5, kMarkerArrayMd5)."""
    table()
    return md5("visualization_msgs/Marker"), md5("visualization_msgs/MarkerArray")


def compressed_image_md5() -> str:
    """md5sum of sensor_msgs/CompressedImage (slam_to_ros.h: kCompressedImageMd5)."""
    table()
    return md5("sensor_msgs/CompressedImage")


if __name__ == "__main__":
    t = table()
    if "--header" in sys.argv[1:]:
        for n in NAMES:
            print('constexpr const char* kMd5%s = "%s";' % (n, t[n]))
        print('constexpr const char* kCompressedImageMd5 = "%s";' % compressed_image_md5())
        print('constexpr const char* kMarkerMd5 = "%s";\nconstexpr const char* kMarkerArrayMd5 = "%s";' % marker_md5s())
    else:
        for n in NAMES:
            print("%s  %s/%s" % (t[n], PACKAGE, n))
