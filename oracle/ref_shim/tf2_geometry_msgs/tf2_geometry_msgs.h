// ref_shim/tf2_geometry_msgs/tf2_geometry_msgs.h — TEST INFRASTRUCTURE ONLY: the inert ROS stand-ins live in one file, ros/ros.h.
#include <ros/ros.h>
