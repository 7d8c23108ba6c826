// ref_shim/tf2/LinearMath/Quaternion.h — TEST INFRASTRUCTURE ONLY: the inert ROS stand-ins live in one file, ros/ros.h.
#include <ros/ros.h>
