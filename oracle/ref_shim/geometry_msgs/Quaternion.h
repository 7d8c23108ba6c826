// ref_shim/geometry_msgs/Quaternion.h — TEST INFRASTRUCTURE ONLY: the inert ROS stand-ins live in one file, ros/ros.h.
#include <ros/ros.h>
