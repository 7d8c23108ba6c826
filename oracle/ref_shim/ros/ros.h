// ref_shim/ros/ros.h — TEST INFRASTRUCTURE ONLY.
//
// Inert stand-ins, of this project's own writing, for the ROS types that the reference's bsplineTraj / astarOcc / utils
// sources name, so that those files compile verbatim (oracle/ref_bspline_harness.cpp).  Nothing here talks to a ROS
// master: publishers and timers do nothing, ros::ok() is always true, and ros::Time::now() is always zero — so the
// reference's wall-clock limits (0.2 s in A*, 0.03 s in optimizeTrajectory) never fire and every run is deterministic.
// NodeHandle::getParam reads a table that the harness fills (ros::shim::params()), so initParam() runs as written.
// The message structs carry the public data members the sources touch, named like the real messages.
#ifndef REF_SHIM_ROS_ROS_H
#define REF_SHIM_ROS_ROS_H
#include <cmath>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#define ROS_ERROR(...) do { } while (0)
#define ROS_WARN(...) do { } while (0)
#define ROS_INFO(...) do { } while (0)

namespace ros {
namespace shim {
inline std::map<std::string, std::vector<double>>& params() {
    static std::map<std::string, std::vector<double>> table;
    return table;
}
}  // namespace shim

inline bool ok() { return true; }

struct Duration {
    double sec;
    Duration() : sec(0) {}
    explicit Duration(double s) : sec(s) {}
    double toSec() const { return sec; }
};
struct Time {
    double sec;
    Time() : sec(0) {}
    static Time now() { return Time(); }
    double toSec() const { return sec; }
};
inline Duration operator-(const Time& a, const Time& b) { return Duration(a.sec - b.sec); }
struct TimerEvent {};
struct Timer {};
struct Publisher {
    template <class M> void publish(const M&) const {}
};
class NodeHandle {
public:
    NodeHandle() {}
    bool getParam(const std::string& key, double& v) const {
        auto it = shim::params().find(key);
        if (it == shim::params().end() || it->second.empty()) return false;
        v = it->second[0];
        return true;
    }
    bool getParam(const std::string& key, bool& v) const {
        double d;
        if (!getParam(key, d)) return false;
        v = d != 0.0;
        return true;
    }
    bool getParam(const std::string& key, int& v) const {
        double d;
        if (!getParam(key, d)) return false;
        v = static_cast<int>(d);
        return true;
    }
    bool getParam(const std::string& key, std::vector<double>& v) const {
        auto it = shim::params().find(key);
        if (it == shim::params().end()) return false;
        v = it->second;
        return true;
    }
    template <class M> Publisher advertise(const std::string&, int) { return Publisher(); }
    template <class T> Timer createTimer(Duration, void (T::*)(const TimerEvent&), T*) { return Timer(); }
};
}  // namespace ros

namespace std_msgs {
struct Header {
    std::string frame_id;
    ros::Time stamp;
};
struct ColorRGBA {
    double r = 0, g = 0, b = 0, a = 0;
};
}  // namespace std_msgs

namespace geometry_msgs {
struct Point { double x = 0, y = 0, z = 0; };
struct Vector3 { double x = 0, y = 0, z = 0; };
struct Quaternion { double x = 0, y = 0, z = 0, w = 1; };
struct Pose {
    Point position;
    Quaternion orientation;
};
struct PoseStamped {
    std_msgs::Header header;
    Pose pose;
};
struct Twist {
    Vector3 linear, angular;
};
}  // namespace geometry_msgs

namespace nav_msgs {
struct Path {
    std_msgs::Header header;
    std::vector<geometry_msgs::PoseStamped> poses;
};
}  // namespace nav_msgs

namespace visualization_msgs {
struct Marker {
    enum { ARROW = 0, CUBE = 1, SPHERE = 2, ADD = 0 };
    std_msgs::Header header;
    std::string ns;
    int id = 0, type = 0, action = 0;
    geometry_msgs::Pose pose;
    geometry_msgs::Vector3 scale;
    std_msgs::ColorRGBA color;
    ros::Duration lifetime;
    std::vector<geometry_msgs::Point> points;
};
struct MarkerArray {
    std::vector<Marker> markers;
};
}  // namespace visualization_msgs

// utils.h's yaw helpers: roll-pitch-yaw <-> quaternion by the textbook formulas (none of the tested paths calls them)
namespace tf2 {
struct Quaternion {
    double x = 0, y = 0, z = 0, w = 1;
    void setRPY(double roll, double pitch, double yaw) {
        const double cr = std::cos(roll / 2), sr = std::sin(roll / 2), cp = std::cos(pitch / 2), sp = std::sin(pitch / 2);
        const double cy = std::cos(yaw / 2), sy = std::sin(yaw / 2);
        x = sr * cp * cy - cr * sp * sy;
        y = cr * sp * cy + sr * cp * sy;
        z = cr * cp * sy - sr * sp * cy;
        w = cr * cp * cy + sr * sp * sy;
    }
};
inline geometry_msgs::Quaternion toMsg(const Quaternion& q) {
    geometry_msgs::Quaternion m;
    m.x = q.x; m.y = q.y; m.z = q.z; m.w = q.w;
    return m;
}
inline void convert(const geometry_msgs::Quaternion& m, Quaternion& q) { q.x = m.x; q.y = m.y; q.z = m.z; q.w = m.w; }
struct Matrix3x3 {
    Quaternion q;
    explicit Matrix3x3(const Quaternion& quat) : q(quat) {}
    void getRPY(double& roll, double& pitch, double& yaw) const {
        roll = std::atan2(2 * (q.w * q.x + q.y * q.z), 1 - 2 * (q.x * q.x + q.y * q.y));
        pitch = std::asin(2 * (q.w * q.y - q.z * q.x));
        yaw = std::atan2(2 * (q.w * q.z + q.x * q.y), 1 - 2 * (q.y * q.y + q.z * q.z));
    }
};
}  // namespace tf2
#endif
